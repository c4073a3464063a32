/*
 * Tuning entry points of the TUNING build of libvda (make tune -> build/tune/libvda.so, -DVDA_TUNING).
 * The product libvda.so has none of them and no mutable global state: its routes are fixed at the
 * automatic choices below (-1 / 0).  Every knob is process-global in the tuning build; it exists for
 * A/B measurements (tools/) and for the tests that check each alternative kernel route against the
 * default one.
 */
#ifndef VDA_TUNE_H
#define VDA_TUNE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* GEMM / conv tile configuration (-1 = automatic; 0 = 128x128/4 waves, 1 = 256x128/8 waves,
 * 2 = 128x64/4 waves, 3 = 256x256/8 waves; -2 / -3 = automatic tiles with the strip-tiled 3x3 conv for
 * no / every Cout = 256 shape; 13 (any value >= 10) = the implicit-GEMM depth tail for every shape, which
 * has one tile configuration and ignores the values below 10).  6 = 64x64 and 7 = 64x128 exist for the dense
 * GEMM only; 4 = 256x256 and 5 = 512x128 are the phased kernels. */
int vda_debug_force_tile(int32_t cfg);
/* Phased 256-row GEMM: persist_blocks > 0 launches that many persistent blocks (0 = one block per tile,
 * -1 = automatic: one per CU). */
int vda_debug_gemm_sched(int32_t persist_blocks);
/* Strip-tiled 3x3 conv: split every tile's input channels over nsplit work items (1, 2, 4, 8; must divide
 * Cin / 32); 0 = automatic. */
int vda_debug_strip_split(int32_t nsplit);
/* Halo-tiled phased 3x3 conv (Cout = 256): -1 = automatic (maps of >= 128^2 pixels), 0 = never,
 * 1 = every shape it serves. */
int vda_debug_hconv(int32_t mode);
/* Depth tail: -1 = automatic (the 2-blocks-per-CU depth conv with the resize fused), 2 = the same conv on
 * a materialised resize (bit-identical; needs the workspace).  Any other value is refused (non-zero return,
 * knob unchanged). */
int vda_debug_dconv(int32_t mode);
/* 3x3 conv with 128 outputs through an exact x2 resize (output_conv1): 1 = automatic (the kernel that mixes the
 * channels at the source resolution, vda_oc1_src.hip, for a call with a bias9 table; a plain-bias call keeps the
 * halo conv with the fused resize and with it the bits of resize + conv), 2 = the source-resolution kernel
 * wherever it serves, 0 = the halo conv with the fused resize for every shape.  Any other value is refused
 * (non-zero return, knob unchanged). */
int vda_debug_oc1_src(int32_t mode);
/* Temporal attention: 1 = the direct-load kernel for every head dim (0 = automatic: the LDS-staged one
 * where it applies). */
int vda_debug_attn(int32_t temporal_direct);

#ifdef __cplusplus
}
#endif
#endif /* VDA_TUNE_H */
