// Host entry points that cross translation units inside libvda (not part of the C ABI of include/vda.h).
// Every file that defines one of these and every file that calls one includes this header, so the two
// sides cannot drift apart.  Return convention of the kernel routes (vda_conv_*, vda_depth_*): 0 = launched,
// 1 = this shape is not served (the router tries its next route), anything else = error.
#pragma once
#include "vda_common.h"
#include "../../include/vda.h"
static_assert(vda_glu(VDA_ACT_GEGLU) && vda_glu(VDA_ACT_SWIGLU) && !vda_glu(VDA_ACT_GELU) && !vda_glu(VDA_ACT_RELU),
              "vda_glu (vda_common.h) names the gated activation codes of vda.h");

// ---- vda_gemm.hip: the MFMA GEMM / implicit-GEMM conv kernels behind plain launch functions ----
struct GemmParams {
  const h16* x; long ldx;
  const h16* w;
  h16* y; long ldy;
  int M, N, K;
  // implicit conv geometry (conv mode only)
  int H, W, Cin, Ho, Wo, ks, stride, pad, pre_relu, up_h, up_w;
  vda_epilogue epi;
  // sub-pixel conv route only (vda_launch_subpixel_gemm; with H, W = the source map and stride = s): frames,
  // the (a << 2 | b) phase of each 256-wide N tile as nibbles, the [9][256] class bias table
  int sp_bt, sp_phases;
  const float* sp_bias;
};
// vda_debug_force_tile (tuning build): tile configuration / route override read by the GEMM launcher and
// by the conv and depth-head routers; -1 = automatic
VDA_KNOB_DECL(int, g_force_tile, -1);
vda_epilogue vda_default_epi();
int vda_check_epi(const vda_epilogue& e, int M, int N);
// dense GEMM / implicit-GEMM conv (activation none / ReLU): launches what the route says, applies p.epi
// (and stats_out)
int vda_launch_gemm(const GemmParams& p, hipStream_t st);
int vda_launch_conv_gemm(const GemmParams& p, hipStream_t st);
// the sizes the phased 256x256 dense kernel serves: X [M, K] of row stride ldx, W [N, K] (the route's own
// term, for a caller that builds X for that kernel)
bool vda_gemm_phased256_serves(long M, long N, long K, long ldx);
// one phase group of the sub-pixel conv (vda_subpixel.hip): the dense phased 256x256 kernel on the corner
// matrix X [M = sp_bt (H + 1) (W + 1), K] (row stride ldx), W [256 nph, K], with the class bias and the
// corner -> output pixel store of gemm256_tile's SUBP epilogue; any M >= 1, K % 64 == 0
int vda_launch_subpixel_gemm(const GemmParams& p, hipStream_t st);
// implicit-GEMM conv whose loader resizes its input bilinearly (p.up_h / p.up_w), register-staged
int vda_launch_conv_reg(const GemmParams& p, hipStream_t st);
// implicit-GEMM depth tail (3x3 C -> 32 hi/lo rows, ReLU, 1x1, ReLU; fp32 depth), 256x64 tiles
int vda_launch_depth_gemm(const GemmParams& p, hipStream_t st);

// ---- vda_oc1.hip: halo-tiled 3x3 conv, Cout = 128 (output_conv1), plain and with the resize fused ----
int vda_conv_halo(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int H, int W, int Cin,
                  int Cout, hipStream_t st);
// bias9: the [9][Cout] class table of vda_epilogue.bias9 in place of bias, or NULL
int vda_conv_halo_fused(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int Hs, int Ws,
                        int H, int W, int Cin, int Cout, hipStream_t st, const float* bias9 = nullptr);
bool vda_conv_halo_fused_serves(int BT, int Hs, int Ws, int H, int W, int Cin, int Cout);

// ---- vda_oc1_src.hip: the same conv through an exact x2 resize, channel mixing at the source resolution ----
// arguments and semantics of vda_conv_halo_fused; serves (H, W) = (2 Hs, 2 Ws), Cin % 64 == 0 (<= 256), Cout = 128,
// in the product for a bias9 call only (a plain-bias call keeps the bits of resize + conv)
bool vda_conv_oc1_src_serves(int BT, int Hs, int Ws, int H, int W, int Cin, int Cout, bool bias9);
int vda_conv_oc1_src(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int Hs, int Ws, int H,
                     int W, int Cin, int Cout, hipStream_t st, const float* bias9 = nullptr);

// ---- vda_dconv.hip: depth-tail conv on the resized map, 2 blocks / CU ----
bool vda_depth_conv_serves(int H, int W, int C);
int vda_depth_conv(const void* U, const void* w1, const float* b1, const float* w2, const float* b2, float* depth,
                   int BT, int H, int W, int C, hipStream_t st);
bool vda_depth_conv_fused_serves(int Hs, int Ws, int H, int W, int C);
int vda_depth_conv_fused(const void* x, const void* w1, const float* b1, const float* w2, const float* b2,
                         float* depth, int BT, int Hs, int Ws, int H, int W, int C, hipStream_t st);

// ---- vda_strip.hip: strip-tiled 3x3 conv, Cout = 256 ----
bool vda_conv_strip_serves(int W, int Cin, int Cout);
long vda_conv_strip_ws_bytes(int BT, int H, int W, int Cin, int Cout);
int vda_conv_strip(const void* x, const void* w, void* y, const float* bias, int relu_out, int pre_relu,
                   const void* res, const void* res2, int BT, int H, int W, int Cin, int Cout, void* ws,
                   long ws_bytes, hipStream_t st);

// ---- vda_hconv.hip: halo-tiled phased 3x3 conv, Cout = 256 ----
bool vda_conv_hconv_serves(int BT, int H, int W, int Cin, int Cout);
int vda_conv_hconv(const void* x, const void* w, void* y, const float* bias, int relu_out, int pre_relu,
                   const void* res, const void* res2, int res2_h, int res2_w, int BT, int H, int W, int Cin, int Cout,
                   hipStream_t st);

// ---- vda_norm.hip: per-row partial statistics of an fp16 matrix (the stats_out fallback) ----
int vda_row_partials_launch(const void* y, int64_t ldy, float* out, int32_t rows, int32_t N, hipStream_t st);

// ---- vda_misc.hip: explicit im2col of a conv input into [BT * Ho * Wo, ks * ks * Cin] ----
int vda_conv_im2col(const void* x, void* a, int BT, int H, int W, int Cin, int Ho, int Wo, int ks, int stride, int pad,
                    hipStream_t st);
