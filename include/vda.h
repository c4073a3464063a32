/*
 * libvda — MI355X (gfx950) kernels for the Video-Depth-Anything clip forward.
 *
 * C ABI: plain pointers, sizes and a hipStream_t passed as void*.  No torch types cross this
 * boundary; the Python host (video-depth-anything_amd/) hands in device pointers it owns.
 * Every entry point returns 0 on success, a negative errno-style code for an invalid argument
 * (-22) or a positive hipError_t for a launch failure; vda_last_error() returns the message.
 * Nothing here throws, allocates device memory or synchronises the stream, so every call can be
 * captured into a hipGraph.
 *
 * Conventions
 *   half   = IEEE fp16 (_Float16), float = fp32.
 *   Activations are token-major / NHWC: a [BT, h, w, C] feature map is a [BT*h*w, C] matrix.
 *   Linear / conv weights are fp16, K (input channel) contiguous; biases are fp32.
 *   Alignment: where an entry point states nothing else, every device pointer is 16-byte aligned at its base
 *   (matrices, maps, weights, qkv, workspaces, and the fp32 per-channel / per-row operands bias, rowbias, gamma,
 *   beta, ln_colsum, ln_stats, stats_out, bias9), and no kernel reads or writes outside the elements the shapes
 *   and row strides name: what lies before an operand, after it and between the rows of a strided view is never
 *   loaded into a result (tests/test_gpu_placement.py places every operand at exactly its stated alignment
 *   between NaN / Inf zones).  vda_gemm also takes y, res and res2 at the 8-byte alignment their N % 4 == 0 row
 *   strides imply (the one-tile kernels then serve the call).
 *
 * The reference (FriedFeid/Video-Depth-Anything @ /root/reference) has no native layer or FFI:
 * its hot path is PyTorch modules.  Each entry point below names the reference code it replaces.
 */
#ifndef VDA_H
#define VDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Epilogue activation codes for vda_gemm / vda_conv2d. */
enum {
  VDA_ACT_NONE = 0,
  VDA_ACT_GELU = 1,  /* exact erf GELU (nn.GELU, dinov2.py:61 act_layer)                 */
  VDA_ACT_GEGLU = 2, /* h * gelu(g); weight rows interleaved in 16-row blocks [h|g]      */
  VDA_ACT_RELU = 3,
  VDA_ACT_SWIGLU = 4 /* h * silu(g) (swiglu_ffn.py: silu(x1) * x2, h = x2, g = x1); rows as GEGLU;
                        silu(v) = v / (1 + exp(-v)) in fp32, finite for every fp16 pre-activation */
};

/* Store layouts for vda_gemm. */
enum {
  VDA_STORE_ROWS = 0,         /* Y[m*ldy + n]                                            */
  VDA_STORE_PIXEL_SHUFFLE = 1 /* ConvTranspose2d(k=s): n=(i*k+j)*Cout+co scattered to NHWC */
};

/*
 * Fused epilogue of a GEMM / conv tile, applied to the fp32 accumulator `acc` of output (m, n):
 *   acc = rstd[m] * (acc - mean[m] * ln_colsum[n])         (LayerNorm fold, when ln_stats is set)
 *   v = acc + bias[n] + rowbias[((m / rdiv) % rmod) * N + n]
 *   v = act(v)
 *   v = res[m*ldres + n] + res2[m*ldres2 + n] + gamma[n] * v      (each term optional)
 * then stored as fp16.  Null pointers disable a term.  With VDA_ACT_GEGLU / VDA_ACT_SWIGLU the GEMM N
 * counts the interleaved [h|g] weight rows and the output has N/2 columns; every rule stated for GEGLU
 * below (N % 32 == 0, no rowbias / res2 / pixel shuffle / stats_out, dense only) holds for SwiGLU too.
 */
typedef struct vda_epilogue {
  const float* bias;     /* [N] or NULL                                                */
  const float* rowbias;  /* [rmod, N] or NULL (patch-embed pos-embed, temporal PE·Wᵀ)  */
  int32_t rdiv, rmod;
  const float* gamma;    /* [N] LayerScale or NULL                                     */
  const void* res;       /* half [M, ldres] or NULL (may alias the output)             */
  int64_t ldres;
  const void* res2;      /* half [M, ldres2] or NULL                                   */
  int64_t ldres2;
  int32_t act;           /* VDA_ACT_*                                                  */
  int32_t store;         /* VDA_STORE_*                                                */
  int32_t ps_k, ps_cout, ps_hin, ps_win; /* pixel-shuffle geometry (store == 1)       */
  /* LayerNorm folded into the GEMM (block.py:84,87 norm1 / norm2 feeding qkv / fc1): X is the raw
   * row stream x, W holds gamma (.) W_ln, bias holds W_ln beta + b, ln_colsum[n] = sum_k W[n, k] (of the
   * fp16 W actually used), and ln_stats[m] = (mean, rstd) of row m from vda_row_stats.  Then
   * rstd (x W^T - mean colsum) + bias = LN(x) W_ln^T + b exactly in real arithmetic.  Row store only, no gamma, activation none / gelu / geglu / swiglu.
   * With a rowbias (the motion-module q/k/v: LN(x) + pe[t] then to_q/k/v, motion_module.py:175,256,
   * 263): bias required, no activation / res / res2 / stats_out, rdiv >= 256, N % 256 == 0, 16-byte
   * aligned x, and a shape the GEMM route gives to the phased 256x256 kernel, whose EK 3 epilogue is
   * the only one that implements the pair (-22 otherwise; vda_gemm_check answers for a shape). */
  const float* ln_stats;  /* [M, 2] or NULL                                              */
  const float* ln_colsum; /* [N]                                                     */
  /* ln_parts > 0: ln_stats instead holds [M, ln_parts, 2] partial (sum, sum of squares) of row m
   * over ln_parts column blocks (as written through stats_out by the GEMM that produced X); the
   * epilogue forms mean = sum / K, var = max(sumsq / K - mean^2, 0), rstd = 1 / sqrt(var + ln_eps).
   * ln_parts <= 4, M * max(ln_parts, 1) >= 2.  No padding is needed past [M, ln_parts, 2]: the kernels
   * never read beyond it.  (A row of more than 1024 channels, ViT-g's 1536 = six parts, takes ln_parts = 0
   * with vda_row_stats passes instead.) */
  int32_t ln_parts;
  float ln_eps;
  /* Producer side: write [M, ceil(N / 256), 2] per-row partial (sum, sum of squares) of the fp16
   * OUTPUT values (after the residual adds) over 256-column blocks, for a following LN-folded GEMM
   * (ln_parts = ceil(N / 256)): the statistics pass over the row stream is never a separate read.
   * Row store, no pixel shuffle, no GEGLU; computed by a separate partial-sum kernel when the GEMM
   * shape does not take the phased 256x256 kernel (then N % 8 == 0, ldy % 8 == 0, y 16-byte aligned).
   * Not available in the fp32 entry points. */
  float* stats_out;
  /* res2_h, res2_w > 0 (vda_conv2d only): res2 is a smaller [BT, res2_h, res2_w, N] map read through a
   * bilinear align_corners=True upsample to the output grid (the FeatureFusionBlock input upsampled by
   * the previous block, blocks.py:156-158, consumed as refinenet1's skip add, blocks.py:146-150),
   * bit-identical to vda_upsample_bilinear + the add; ldres2 is then the source row stride (= N).
   * Served where vda_conv2d_res2_upsample_ok says so (the halo-tiled 256-channel conv); 0 = same grid. */
  int32_t res2_h, res2_w;
  /* Optional tile scheduler of the persistent 256x256 GEMM: 9 int32, zero before the first launch and
   * left zero by every launch (the last block to finish clears them).  Blocks then take their tiles
   * beyond the first round by atomic ticket (per XCD) instead of a fixed stride, so blocks that start
   * late (the GPU shared with another stream's kernels) run fewer tiles.  A counter set must not be used
   * by two launches that can run at the same time (one per stream).  NULL: static schedule.  Ignored by
   * the other kernel routes. */
  int32_t* sched;
  /* drop_period > 0 (vda_gemm only): X is a token stream of frames of drop_period rows whose first row is
   * the cls token (the encoder output, dinov2.py:309-312 get_intermediate_layers drops it); output rows
   * m with m % drop_period == 0 are not stored and row m goes to Y row m - m / drop_period - 1, so Y
   * holds the M - ceil(M / drop_period) patch rows.  For the DPT projects 1x1 conv on a tap with the
   * final LayerNorm folded in (dpt.py:60-68).  Served by the phased route's register epilogue only:
   * drop_period >= 256, ln_stats + ln_colsum + bias, activation none, row store, no gamma / res / res2 /
   * rowbias / stats_out, N % 256 == 0, and a shape the GEMM route gives to the phased 256x256 kernel;
   * -22 otherwise (vda_gemm_check answers for a shape). */
  int32_t drop_period;
  /* bias9 (vda_conv2d with up_h / up_w only): a [9][N] fp32 table used INSTEAD of `bias`, one row per class
   * (top / middle / bottom row of the output map) x (left / middle / right column), row 3 r + c: the bias of a
   * 3x3 zero-padded conv composed with a biased 1x1 conv in front of it (refinenet1's out_conv, blocks.py:160,
   * then the x2 resize, whose weights sum to 1, then output_conv1, dpt.py:117): the 1x1 bias reaches an output
   * pixel only through the taps the padding leaves in bounds, bias9[class] = b_1 + sum_{in-bounds t} W_1[t] b_o.
   * Only the outermost ring of output pixels differs from the middle class.  Served by the halo conv with the
   * fused resize alone (vda_conv2d_bias9_ok says for which shapes; -22 elsewhere).  NULL: `bias`. */
  const float* bias9;
} vda_epilogue;

/* Version / diagnostics. */
const char* vda_version(void);
/* sizeof(vda_epilogue) as compiled into the library (bindings check their mirror against it). */
int64_t vda_epilogue_size(void);
const char* vda_last_error(void);

/*
 * Y[M, N] = epilogue( X[M, K] · W[N, K]ᵀ ).   fp16 in/out, fp32 accumulate, MFMA 16x16x32.
 * Replaces every nn.Linear / 1x1 nn.Conv2d / ConvTranspose2d(k=s) of the hot path:
 *   dinov2_layers/attention.py:72,79 (qkv, proj); mlp.py:36-39 (fc1+GELU, fc2); block.py:84-87
 *   (ls1/ls2 LayerScale + residual); dpt.py:60-68 (projects), dpt.py:70-82 (ConvT k4s4/k2s2);
 *   blocks.py:124-126,160 (out_conv); motion_module.py:119,127 (proj_in/out + residual);
 *   motion_module.py:263,272-273 (to_q/k/v with the PE add :256 folded as a per-frame rowbias);
 *   attention.py:328 (to_out); attention.py:374-384 (GEGLU) and :338 (ff out);
 *   dinov2_layers/swiglu_ffn.py (ViT-g: w12 + SwiGLU, w3).
 * Requires K % 8 == 0, ldx % 8 == 0, N % 4 == 0 (N % 32 == 0 for GEGLU / SwiGLU).
 */
int vda_gemm(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy,
             int32_t M, int32_t N, int32_t K, const vda_epilogue* epi, void* stream);
/* vda_gemm's argument and route checks without a launch, for 16-byte aligned x / w / y: 0, or the error
 * vda_gemm would return (message in vda_last_error).  Of each epilogue pointer only whether it is NULL and
 * its alignment are looked at, so stand-in values will do.  A caller with a choice (drop_period or a
 * LayerNorm + GEMM pair, ln_stats + rowbias or LayerNorm first) asks here instead of copying the
 * conditions; vda_gemm itself is this check followed by the launch. */
int vda_gemm_check(int64_t ldx, int64_t ldy, int32_t M, int32_t N, int32_t K, const vda_epilogue* epi);

/*
 * NHWC implicit-GEMM 2-D convolution, fp16 MFMA, square kernel `ks`, zero padding `pad`.
 * X [BT, H, W, Cin] half; Wt [Cout, ks, ks, Cin] half; Y [BT, Ho, Wo, Cout] half.
 * pre_relu applies ReLU to X as it is loaded (ResidualConvUnit, blocks.py:78).
 * Replaces blocks.py:20-32 (layerN_rn 3x3 no bias), blocks.py:78-91 (RCU conv1/conv2 + skip
 * add), blocks.py:146-150 (fusion skip add, via res2), dpt.py:83-89 (3x3 s2 resize), and
 * dpt.py:117 (output_conv1).  Requires Cin % 8 == 0, Cout % 4 == 0.
 * If `up_h`/`up_w` > 0, X is read through a bilinear align_corners=True upsample from
 * [BT, H, W, Cin] to [BT, up_h, up_w, Cin] (blocks.py:156-158 / dpt_temporal.py:92-94), and the
 * conv runs on the upsampled grid.
 * `ws` / `ws_bytes`: a device workspace of vda_conv2d_workspace(...) bytes lets the strip-tiled
 * 3x3 kernel split small maps' input channels over several work items (fp32 partial slices summed
 * in a fixed order: deterministic).  NULL / 0 runs the same conv unsplit.  The library keeps no
 * mutable device state of its own, so calls on different streams with their own workspaces may
 * run concurrently.
 */
int vda_conv2d(const void* x, const void* w, void* y, int32_t BT, int32_t H, int32_t W,
               int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad,
               int32_t pre_relu, int32_t up_h, int32_t up_w, const vda_epilogue* epi,
               void* ws, int64_t ws_bytes, void* stream);
int64_t vda_conv2d_workspace(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks,
                             int32_t stride, int32_t pad);
/* 1 when vda_conv2d of this shape takes an epilogue res2 through the fused upsample (res2_h/res2_w),
 * else 0 (the caller materialises the upsample with vda_upsample_bilinear instead). */
int vda_conv2d_res2_upsample_ok(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks,
                                int32_t stride, int32_t pad);
/* 1 when the 3x3 / stride 1 / pad 1 vda_conv2d of X [BT, H, W, Cin] through the resize to (up_h, up_w) takes a
 * 9-class bias table (vda_epilogue.bias9), else 0 (the caller keeps the 1x1 conv and the plain bias). */
int vda_conv2d_bias9_ok(int32_t BT, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t up_h, int32_t up_w);

/*
 * Sub-pixel conv: ConvTranspose2d(kernel = stride = s, bias) followed by a zero-padded 3x3 conv (no bias),
 * composed by the caller into one linear map of the low-resolution input (dpt.py:70-82 resize_layers[0] / [1]
 * then blocks.py:20-32 layer1_rn / layer2_rn; nothing stands between the two in dpt_temporal.py:55-69, :71-80).
 * X [BT, h, w, Cin] half -> Y [BT, s h, s w, Cout] half, written once; the [BT, s h, s w, Cin] map between the two
 * convs never exists.  With Wt[a][b] the ConvT taps, Wr[dy][dx] the 3x3 weights and p = X zero outside its own
 * frame, for a, b in [0, s):
 *   Y[s i + a, s j + b] = sum_{di, dj in {-1, 0, 1}} Wc[a][b][di][dj] p[i + di, j + dj] + bias9[class(y, x)]
 *   Wc[a][b][di][dj] = sum over (dy, dx) with floor((a + dy) / s) = di, floor((b + dx) / s) = dj of
 *                      Wr[dy][dx] Wt[(a + dy) mod s][(b + dx) mod s]^T                        ([Cout, Cin])
 * Phase a = 0 uses di in {-1, 0}, a = s - 1 uses {0, +1}, the phases between use di = 0 only (columns alike), so
 * a phase sees a 1x1, 1x2, 2x1 or 2x2 window.  The phases are served in groups of four of one window shape; `w`
 * holds the groups one after the other, each [4 * Cout, K] half (K contiguous), rows (phase in the order listed,
 * co), K = the window's source pixels (in the order listed, as (di, dj) relative to the phase's own (i, j)) x Cin:
 *   s = 2: one group, phases (0,0) (0,1) (1,0) (1,1), window pixels (ci-1, cj-1) (ci, cj-1) (ci, cj) (ci-1, cj)
 *          of corner ci = i + a, cj = j + b, i.e. (di, dj) = (r + a, c + b) for corner-relative (r, c) in
 *          (-1,-1) (0,-1) (0,0) (-1,0)
 *   s = 4: 2x2: phases (0,0) (0,3) (3,0) (3,3), the four corner pixels as above with corner (i + [a == 3], j + [b == 3])
 *          1x2: phases (1,0) (1,3) (2,0) (2,3), pixels (ci, cj-1) (ci, cj)
 *          2x1: phases (0,1) (0,2) (3,1) (3,2), pixels (ci, cj) (ci-1, cj)
 *          1x1: phases (1,1) (1,2) (2,1) (2,2), pixel (ci, cj)
 * bias9 [9][Cout] float: the ConvT bias pushed through the in-bounds taps of the 3x3 conv, per class
 * (top / middle / bottom row of Y) x (left / middle / right column): bias9[3 r + c] = sum of Wr[dy][dx] bt over the
 * taps the zero padding leaves at that class.  Added in fp32 before the one rounding to fp16.
 * Route: a corner im2col of X into ws ([BT (h+1) (w+1), 4 Cin] half, vda_subpixel_conv_workspace bytes), then one
 * launch of the phased 256x256 GEMM per group on a K slice of it.  Cout == 256, Cin % 64 == 0, s in {2, 4}, all
 * buffers 16-byte aligned and below 2 GiB; vda_subpixel_conv_check returns 0 for a shape that is served, else -22
 * (message in vda_last_error), without a launch.  fp16 only.
 */
int vda_subpixel_conv(const void* x, const void* w, const float* bias9, void* y, int32_t BT, int32_t h, int32_t w_,
                      int32_t Cin, int32_t Cout, int32_t s, void* ws, int64_t ws_bytes, void* stream);
int64_t vda_subpixel_conv_workspace(int32_t BT, int32_t h, int32_t w_, int32_t Cin, int32_t s);
int vda_subpixel_conv_check(int32_t BT, int32_t h, int32_t w_, int32_t Cin, int32_t Cout, int32_t s);

/*
 * Row LayerNorm, fp32 statistics.  X rows of C halfs (row stride ldx); Y [rows, C] half.
 * With skip_period > 0, output row r reads input row r + r/(skip_period) + 1, i.e. it drops the
 * cls token of every [1+skip_period]-token frame (dinov2.py:309-312).
 * Replaces block.py:84,87 (norm1/norm2, eps 1e-6), dinov2.py:310 (final norm on the taps),
 * motion_module.py:175,183 (temporal LayerNorms, eps 1e-5).
 */
int vda_layernorm(const void* x, int64_t ldx, void* y, const float* gamma, const float* beta,
                  int32_t rows, int32_t C, float eps, int32_t skip_period, void* stream);

/*
 * Per-row LayerNorm statistics for the LN-folded GEMM (vda_epilogue.ln_stats): stats[r] = (mean,
 * 1/sqrt(var + eps)) of row r of X (rows of C halfs, row stride ldx), fp32, two-pass like
 * vda_layernorm (same values).  Replaces the statistics half of block.py:84,87 (norm1 / norm2).
 */
int vda_row_stats(const void* x, int64_t ldx, float* stats, int32_t rows, int32_t C, float eps,
                  void* stream);

/*
 * GroupNorm over NHWC frames: X [F, S, C] half -> Y [F, S, C] half, `groups` groups of C/groups
 * channels, statistics over (S x C/groups) in fp32.  `ws`: a float workspace of
 * vda_groupnorm_workspace(F, S, C, groups) entries enables the three-pass coalesced path
 * (per row-chunk and channel the mean and the centred second moment, two-pass from registers; their
 * parallel-variance merge per (frame, group); apply; deterministic); NULL runs the
 * one-block-per-(frame, group) two-pass kernel.  Both take every second moment about the mean of the
 * values it sums, so a massive activation anywhere in the frame cannot cancel the variance.  The
 * workspace holds no input: the call writes all of it that it reads.
 * Replaces motion_module.py:116 (GroupNorm(32, eps 1e-6)).
 */
int vda_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int32_t F,
                  int32_t S, int32_t C, int32_t groups, float eps, float* ws, void* stream);
int64_t vda_groupnorm_workspace(int32_t F, int32_t S, int32_t C, int32_t groups);

/*
 * GroupNorm -> Linear: Y [F*S, N] = GN(X) · Wᵀ + bias, X [F, S, C] half, W [N, C] half, gamma / beta /
 * bias fp32 (bias may be NULL), Y half.  Replaces motion_module.py:116-119 (self.norm(hidden_states),
 * the (b f) c h w -> (b f) (h w) c rearrange, self.proj_in) - the op SURVEY.md §8(b) names
 * groupnorm_linear.  For groups == 32 and N == C in {64, 128, 256} (every motion module of the
 * shipped encoders) the normalisation is applied to the GEMM operand in registers (no normalised copy
 * of X in HBM): W' = fp16(W diag(gamma)) and W beta + bias are formed per block in LDS, and the operand
 * is fp16((x - mean) rstd); other shapes run vda_groupnorm + vda_gemm through the workspace
 * (vda_groupnorm_linear_fused says which; ViT-L's C = 1024 modules take this route).  stats_out
 * (optional): [F*S, ceil(N / 256), 2] per-row (sum, sum of squares) of the stored fp16 rows over
 * 256-column blocks, as vda_epilogue.stats_out.  ws: a 16-byte aligned
 * device buffer of at least vda_groupnorm_linear_workspace(...) bytes.  x, w, y 16-byte aligned.
 */
int vda_groupnorm_linear(const void* x, const float* gamma, const float* beta, int32_t F, int32_t S,
                         int32_t C, int32_t groups, float eps, const void* w, const float* bias, void* y,
                         int32_t N, float* stats_out, void* ws, int64_t ws_bytes, void* stream);
int64_t vda_groupnorm_linear_workspace(int32_t F, int32_t S, int32_t C, int32_t groups, int32_t N);
int vda_groupnorm_linear_fused(int32_t C, int32_t groups, int32_t N);

/*
 * Spatial multi-head self-attention (flash / online softmax, fp16 MFMA, fp32 softmax).
 * qkv [B*N, 3*H*D] half laid out as [B, N, 3, H, D] (the nn.Linear qkv output);
 * out [B*N, H*D] half.  D must be 64.  Replaces dinov2_layers/attention.py:49-62/:65-81
 * (softmax(q kᵀ / sqrt(D)) v; xformers memory_efficient_attention BMHK).
 */
int vda_spatial_attention(const void* qkv, void* out, int32_t B, int32_t N, int32_t H,
                          int32_t D, float scale, void* stream);

/*
 * Temporal self-attention across T <= 32 frames at every spatial site.
 * qkv [(B*T)*S, 3*H*D] half (frame-major rows, [q|k|v] columns, heads contiguous);
 * out [(B*T)*S, H*D] half.  D % 8 == 0, D <= 192 (192 = the ViT-g head's motion modules, C = 1536).
 * D in {32, 64, 128, 192} with H a multiple of the kernel's waves per block (4, 4, 2, 2) runs a kernel that
 * stages q, k, v in LDS; every other case one that loads its fragments from HBM directly.
 * rope_theta > 0 applies the rotary embedding of pe='rope' to q and k first: channel pairs
 * (2i, 2i+1) of all C = H*D channels of frame t rotate by t * rope_theta^(-2i/C), in fp32 from the
 * fp16 q/k, rounded back to fp16 (attention.py:403-429, motion_module.py:290-293); 0 = none ('ape',
 * whose additive table the caller folds into the q/k/v GEMM as a row bias).
 * Replaces motion_module.py:247-335 (rearrange (b f) d c -> (b d) f c, 8-head softmax over f,
 * rearrange back) and attention.py:182-211/:256-293.
 */
int vda_temporal_attention(const void* qkv, void* out, int32_t B, int32_t T, int32_t S,
                           int32_t H, int32_t D, float scale, float rope_theta, void* stream);

/*
 * Bilinear resize, align_corners=True, NHWC half: X [BT, H, W, C] -> Y [BT, Ho, Wo, C].
 * Replaces blocks.py:156-158 and dpt_temporal.py:92-94 where not fused into a conv.
 */
int vda_upsample_bilinear(const void* x, void* y, int32_t BT, int32_t H, int32_t W, int32_t C,
                          int32_t Ho, int32_t Wo, void* stream);

/*
 * Patch-embed im2col: images [BT, 3, H, W] float (NCHW, as VideoDepthAnything.forward receives
 * them) -> A [BT*(1+np), Kp] half with np = (H/14)*(W/14), K order (ci, ky, kx), zero-padded to
 * Kp >= 588, and an all-zero row 0 per frame for the cls token.  Followed by vda_gemm with a
 * per-token rowbias this replaces patch_embed.py:69-82 + dinov2.py:212-219 (cls cat, pos add).
 * img must be 8-byte aligned and a 16-byte aligned (vector loads / stores); -22 otherwise.
 */
int vda_patch_im2col(const float* img, void* a, int32_t BT, int32_t H, int32_t W, int32_t Kp,
                     void* stream);

/*
 * Depth head tail (dpt_temporal.py:92-99, dpt.py:118-124, video_depth.py:63-64):
 * X [BT, Hin, Win, C] half (the output_conv1 result) is bilinearly resized (align_corners=True,
 * fp16 storage like the reference's autocast interpolate), then conv3x3(C -> 32, +b1) -> ReLU ->
 * conv1x1(32 -> 1, w2, +b2) -> ReLU.  The resize is normally fused into the conv's patch staging
 * (the resized map is never written); shapes that need it materialised use the caller's workspace
 * ws [BT, Ho, Wo, C] half of vda_depth_head_workspace(...) bytes (0 = not needed: ws may be NULL).
 * The 3x3 conv keeps fp32 weights as an exact fp16 hi/lo split: w1 is half [64, 3, 3, C] with
 * rows 0..31 = fp16(w) and rows 32..63 = fp16(w - fp16(w)); both halves accumulate in fp32.
 * depth [BT, Ho, Wo] float.  C % 8 == 0.
 */
int vda_depth_head(const void* x, const void* w1, const float* b1, const float* w2,
                   const float* b2, float* depth, void* ws, int32_t BT, int32_t Hin, int32_t Win,
                   int32_t C, int32_t Ho, int32_t Wo, void* stream);
int64_t vda_depth_head_workspace(int32_t BT, int32_t Hin, int32_t Win, int32_t C, int32_t Ho, int32_t Wo);

/*
 * Frame preprocessing on the device: uint8 RGB frames [N, h, w, 3] (HWC) -> float [N, 3, H, W]
 * = (bicubic_resize(frames / 255) - mean[c]) / std[c].  Bicubic a = -0.75, half-pixel centres,
 * clamped borders, no antialias (cv2.INTER_CUBIC; torch interpolate bicubic align_corners=False).
 * mean / std: 3 floats each in HOST memory.  Replaces util/transform.py:5-157 (Resize with
 * keep_aspect_ratio / lower_bound / multiple 14 chooses H, W on the host; NormalizeImage;
 * PrepareForNet) as video_depth.py:336-361 and :140-146, :209 apply them per frame.
 */
int vda_preprocess_frames(const void* frames, float* out, int32_t N, int32_t h, int32_t w, int32_t H,
                          int32_t W, const float* mean, const float* std, void* stream);

/*
 * Depth resize to the source frame size: depth [N, H, W] float -> out [N, ho, wo] float, bilinear
 * align_corners=True.  Replaces video_depth.py:372 (infer_video_depth) and :300 (streaming).
 */
int vda_depth_resize(const float* depth, float* out, int32_t N, int32_t H, int32_t W, int32_t ho,
                     int32_t wo, void* stream);

/*
 * Least-squares scale/shift of pred onto target over n elements, on the device:
 *   a_00 = S m p^2, a_01 = S m p, a_11 = S m, b_0 = S m p t, b_1 = S m t   (m = mask, NULL = all ones)
 *   det = a_00 a_11 - a_01^2
 *   ss = (scale, shift) = ((a_11 b_0 - a_01 b_1) / det, (-a_01 b_0 + a_00 b_1) / det), or (1, 0) when det == 0.
 * Every sum and the solve are fp64 in a fixed order (no atomics: the same input gives the same bits on
 * every run); ss is rounded to fp32 on the store only.  sums [5] double (a_00, a_01, a_11, b_0, b_1) and
 * ss [2] float are DEVICE memory; sums may be NULL.  pred / target: any 4-byte-aligned address, n >= 1.
 * ws: vda_scale_shift_workspace(n) bytes of device memory, 8-byte aligned, owned by the caller; it needs
 * no initialisation and holds nothing between calls.  No synchronisation: the result stays on the device.
 * Replaces compute_scale_and_shift (utils/util.py:40-62) as called from video_depth.py:393-395 (long
 * video) and :312-314 (streaming), which sum in fp32 on the host.
 */
int64_t vda_scale_shift_workspace(int64_t n);
int vda_scale_shift(const float* pred, const float* target, const uint8_t* mask, int64_t n, double* sums,
                    float* ss, void* ws, int64_t ws_bytes, void* stream);

/*
 * Resize + align + blend in one pass: per output pixel of out [F, ho, wo]
 *   r = bilinear align_corners=True resize of src [F, H, W] (the arithmetic of vda_depth_resize)
 *   v = r * ss[0] + ss[1]          (multiply and add rounded separately; ss DEVICE [2], NULL = identity)
 *   v = v < 0 ? 0 : v              (when clip != 0)
 *   out = pre * w_pre[f] + v * w_post[f]   (three roundings; pre [F, ho, wo] or NULL: out = v)
 * w_pre / w_post: F floats each in HOST memory (needed with pre only); out may alias pre.  F <= 32.
 * Replaces video_depth.py:371 + :400-413 with get_interpolate_frames (utils/util.py:65-73) for the long
 * video and :299 + :315 for streaming (which does not clip).
 */
int vda_depth_align(const float* src, int32_t F, int32_t H, int32_t W, int32_t ho, int32_t wo, const float* ss,
                    int32_t clip, const float* pre, const float* w_pre, const float* w_post, float* out,
                    void* stream);

/*
 * Ground-truth evaluation on the device (the reference's eval.py:149-181): pred [F, S] float is the model's
 * relative inverse depth, gt [F, S] float metres, valid [F, S] uint8 (non-zero = valid, NULL = all valid),
 * S = h * w elements per frame, frames at f * S.  Both entry points are streaming reductions in the manner of
 * vda_scale_shift: every per-pixel operation is one correctly rounded fp32 operation (-, /, *, compare,
 * select; no reciprocal approximation, no contraction), every sum is fp64 in a fixed order (per thread ->
 * wave -> block -> a frame's block partials in index order -> frames in frame order), so the same input
 * gives the same bits on every run, and frame f of an [F, S] call gets the bits of a single-frame call on
 * it.  Invalid pixels are selected out, not multiplied out: gt may be 0 or NaN there and reaches no sum.
 * No atomics, no allocation, no synchronisation; the results stay on the device.  1 <= F <= 65535 (the
 * launch grid), S >= 1, pred / gt / ss / aligned 4-byte aligned, the double arrays and ws 8-byte aligned.
 * ws: vda_depth_eval_workspace(F, S) bytes of device memory owned by the caller; it needs no
 * initialisation and holds nothing between calls.
 *
 * vda_depth_eval_fit: G = per_frame ? F : 1 least-squares fits in inverse depth over the valid pixels,
 *   minimise S (c0 pred + c1 - t)^2, t = 1 / gt (an fp32 division), from
 *   sums [G, 5] double (may be NULL) = (S p^2, S p, S 1, S p t, S t), det = a_00 a_11 - a_01^2,
 *   c0 = (a_11 b_0 - a_01 b_1) / det, c1 = (-a_01 b_0 + a_00 b_1) / det in fp64, and
 *   ss [G, 2] float = (scale, shift) = (1 / c0, -c1 / c0), rounded to fp32 once, on the store.
 *   Replaces align_prediction's fit (utils/align.py:192-207 -> frame_aligning_scale_shift_lstsq, :151-160),
 *   which gathers the valid pixels into an [n_valid, 2] matrix on the host for an SVD lstsq.
 *   Deviation: with no valid pixel, det == 0 (e.g. a constant pred) or c0 == 0 the result is (inf, 0), and
 *   every aligned pixel becomes max_depth; the reference does this for c0 == 0 only, its lstsq returns a
 *   minimum-norm solution in the other two cases.
 *
 * vda_depth_eval_metrics: with (scale, shift) = ss[ss_per_frame ? f : 0], per pixel in fp32
 *   a = clip((pred - shift) / scale, 0, 1);  a = a == 0 ? 1e-4f : a;  p = clip(1 / a, 0, max_depth)
 *   (utils/align.py:210-216; clip lets NaN through as numpy's does), and over the valid pixels with
 *   g = gt, d = p - g:
 *   frame_sums [F, 8] double = (count, #{max(p/g, g/p) > 1.25}, #{.. > 1.5625}, #{.. > 1.953125},
 *                               S d/g, S |d|, S |d|/g, S d*d)      (the terms are fp32, the sums fp64)
 *   total [8] double (may be NULL) = frame_sums added in frame order;
 *   aligned [F, S] float (may be NULL) = p of every pixel, valid or not.  max_depth > 0.
 *   Delta_k = 1 - sums[k] / count, SignedRelative = sums[4] / count, AbsoluteError = sums[5] / count,
 *   AbsoluteRelative = sums[6] / count, MeanSquaredError = sums[7] / count: utils/metrics.py:24-31, :91-192,
 *   ten full-size host passes in the reference.
 *   Deviation: under numpy >= 2 the reference's scale is a float64 scalar, which promotes its aligned map
 *   and every metric to float64; under numpy 1.x the same code stays in float32.  Here the per-pixel
 *   arithmetic is fp32 always, so `aligned` equals the separate torch fp32 ops bit for bit.
 */
int64_t vda_depth_eval_workspace(int32_t F, int64_t S);
int vda_depth_eval_fit(const float* pred, const float* gt, const uint8_t* valid, int32_t F, int64_t S,
                       int32_t per_frame, double* sums, float* ss, void* ws, int64_t ws_bytes, void* stream);
int vda_depth_eval_metrics(const float* pred, const float* gt, const uint8_t* valid, int32_t F, int64_t S,
                           const float* ss, int32_t ss_per_frame, float max_depth, float* aligned,
                           double* frame_sums, double* total, void* ws, int64_t ws_bytes, void* stream);

/*
 * Depth visualisation on the device (the reference's save_video, utils/dc_utils.py:72-89): the clip-wide
 * min / max, then fp32 depth straight to the bytes of the output file through a 256-row table.  No atomics,
 * no allocation, no synchronisation; results stay on the device.
 *
 * vda_depth_range: range [2] float (DEVICE) = (min, max) of the n >= 1 floats at depth (dc_utils.py:76).  A
 *   two-stage reduction (block partials in ws, then one block) with 16-byte loads on the aligned body; depth
 *   needs 4-byte alignment only.  NaNs are skipped (fminf / fmaxf); an all-NaN input gives (+inf, -inf).
 *   n is 64-bit.  ws: vda_depth_range_workspace(n) bytes of device memory owned by the caller, 4-byte
 *   aligned; it needs no initialisation and holds nothing between calls.
 *
 * vda_depth_colorize: per pixel of depth [F, H, W] in fp32, every operation correctly rounded (IEEE
 *   division, no reciprocal, no contraction):
 *     x = (d - range[0]) / (range[1] - range[0]) * 255.0f;   i = (uint8_t)x by truncation
 *   which is dc_utils.py:79 as numpy float32 computes it, then out = lut[i] in `layout`.  range [2] float
 *   (DEVICE) may have been computed over another, larger tensor than depth (the range of the whole video,
 *   the colouring per chunk).  lut [256, 3] uint8 (DEVICE, any alignment) is staged once per block in LDS;
 *   the kernel does not know colour spaces: pass RGB rows for RGB output, already converted YUV rows for
 *   y4m payloads.
 *   Deviation: x that is NaN (a constant clip gives 0 / 0) or below 0 gives index 0, x above 255 gives 255;
 *   numpy's cast is undefined there (on x86 it gives 0 for the constant clip, as here).
 *   Layouts (out holds vda_depth_colorize_bytes(F, H, W, layout) bytes, nothing is written outside them):
 *     VDA_VIS_INDEX      [F, H, W]      the index itself; lut may be NULL
 *     VDA_VIS_HWC        [F, H, W, 3]   lut[i] interleaved (what Pillow and imageio take)
 *     VDA_VIS_PLANAR444  [F, 3, H, W]   plane c holds lut[i][c]: the payload of a y4m C444 frame
 *     VDA_VIS_PLANAR420  [F, H*W + 2*ch*cw], ch = (H+1)/2, cw = (W+1)/2: per frame the full-size plane 0, then
 *                        planes 1 and 2 subsampled, each sample (a + b + c + d + 2) >> 2 over the 2x2 block of
 *                        looked-up values, the last row / column repeated at odd sizes (an exact integer
 *                        reduction): the payload of a y4m C420 frame
 *   Neither depth (4-byte aligned) nor out (any address) needs 16-byte alignment: every frame and plane has
 *   its own bytewise head and tail (at most 3 pixels each) around dword stores.  In the 4:2:0 layout a strip
 *   of 8 x 2 pixels is stored as dwords when its row address is dword-aligned, and with bytes and 16-bit
 *   words around a dword otherwise (never at W % 8 == 0 with a 4-byte-aligned out).  1 <= F <= 65535 (the
 *   launch grid), H, W >= 1.
 */
enum {
  VDA_VIS_INDEX = 0,
  VDA_VIS_HWC = 1,
  VDA_VIS_PLANAR444 = 2,
  VDA_VIS_PLANAR420 = 3
};
int64_t vda_depth_range_workspace(int64_t n);
int vda_depth_range(const float* depth, int64_t n, float* range, void* ws, int64_t ws_bytes, void* stream);
int64_t vda_depth_colorize_bytes(int32_t F, int32_t H, int32_t W, int32_t layout);
int vda_depth_colorize(const float* depth, int32_t F, int32_t H, int32_t W, const float* range,
                       const uint8_t* lut, int32_t layout, uint8_t* out, void* stream);

/*
 * Point clouds on the device (the reference's project_image_to_pointcloud / project_scene_to_3d,
 * datasets/visualisation_utils.py:82-187, which go through Open3D on the host): metric depth through the
 * pinhole intrinsics and one affine matrix per frame to a dense, ordered list of 3-D points, as tensors or as
 * the body of a binary PLY.  An order-preserving stream compaction fused with the unprojection, in two calls.
 * No atomics, no allocation, no synchronisation; results stay on the device; argument checks (-22) run before
 * any launch.
 *
 * Operands: depth [F, H, W] float (metres, 4-byte aligned); valid [F, H, W] uint8 (non-zero = valid) or NULL
 * (all valid, as in the reference, whose mask line is commented out); rgb [F, H, W, 3] uint8 or NULL;
 * K [F, 4] float = (fx, fy, cx, cy); M [F, 3, 4] float, row-major camera-to-output, or NULL (none).
 * 1 <= F <= 65535 (the launch grid), H, W, step >= 1, at most 2^31 - 1 candidates per frame.
 * Candidates of frame f: the pixels (i, j) with i % step == 0 and j % step == 0, row-major, frames in index
 * order.  A candidate is kept when (valid == NULL || valid[f,i,j] != 0) && d > 0.0f && d < trunc, d =
 * depth[f,i,j]: NaN, +-Inf, zero and negative depths fail the compares; they are selected out, never
 * multiplied out.  trunc: the reference passes the double max_depth - 1e-4 to Open3D, which compares the
 * float pixel against it; pass the smallest float >= that double and the fp32 compare decides the same.
 * Point of a kept candidate, every operation one correctly rounded fp32 operation (IEEE division, no
 * reciprocal, no contraction), with the original i and j:
 *   z = d;  x = ((float)j - cx) * z / fx;  y = ((float)i - cy) * z / fy
 *   out_r = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3],  r = 0, 1, 2        (M == NULL: x, y, z)
 * so the result equals the separate torch fp32 ops bit for bit.  Colour: the three bytes of rgb[f,i,j].
 * Deviation: Open3D computes in double and divides by the homogeneous w; here M is affine and fp32.
 * The kept points are output densely in candidate order.  The same input gives the same bytes on every run,
 * and frame f of an [F] call gets the bits of a single-frame call on it.
 *
 * vda_cloud_count: a block owns one contiguous run of vda_cloud_span() candidates of one frame and counts
 *   the ones it keeps; a scan per frame and one over the frames give frame_offsets [F + 1] int64 (DEVICE,
 *   8-byte aligned) = the exclusive prefix of the frames' counts, frame_offsets[F] = the total N.
 *   ws: exactly vda_cloud_workspace(F, H, W, step) bytes of device memory owned by the caller, 8-byte
 *   aligned; it needs no initialisation.  Unlike the other workspaces of this library it CARRIES STATE: count
 *   leaves every block's output offset in it and vda_cloud_write reads them, so hand the same, untouched ws
 *   (and the same depth, valid, F, H, W, step, trunc) to write.
 * vda_cloud_write: recomputes the predicate, ranks the kept lanes of a wave with the 64-bit ballot, adds the
 *   wave bases through LDS and the block's offset from ws, and stores the points with index < cap only:
 *   nothing is written at or past cap (cap >= 0; cap = N writes everything) and nothing outside the output.
 *     VDA_CLOUD_SPLIT    out float [cap, 3] (4-byte aligned) and, with rgb, out_rgb uint8 [cap, 3] (any
 *                        address; must be non-NULL when rgb is)
 *     VDA_CLOUD_PACKED   out = cap records of 12 bytes (float x y z) or, with rgb, 15 bytes (float x y z,
 *                        uchar r g b), little-endian: the body of a binary PLY.  out may have ANY byte
 *                        alignment; out_rgb is not used.
 *   A block's records are staged in LDS and leave as one contiguous byte run: bytes up to the first dword
 *   boundary, dword stores, bytes after the last one.
 */
enum {
  VDA_CLOUD_SPLIT = 0,
  VDA_CLOUD_PACKED = 1
};
int64_t vda_cloud_workspace(int32_t F, int32_t H, int32_t W, int32_t step);
int64_t vda_cloud_span(void);
int vda_cloud_count(const float* depth, const uint8_t* valid, int32_t F, int32_t H, int32_t W, int32_t step,
                    float trunc, int64_t* frame_offsets, void* ws, int64_t ws_bytes, void* stream);
int vda_cloud_write(const float* depth, const uint8_t* valid, const uint8_t* rgb, int32_t F, int32_t H, int32_t W,
                    int32_t step, float trunc, const float* K, const float* M, int32_t layout, void* out,
                    uint8_t* out_rgb, int64_t cap, const void* ws, int64_t ws_bytes, void* stream);

/*
 * Ground-truth comparison video on the device (the reference's calculate_metrics.py:206-258 with
 * utils/vis_util.py: visualise_data): per frame a canvas of rows x cols tiles of H x W pixels, the RGB frame,
 * the GT depth, and per method an error map |gt - pred|, the prediction and a "stability" image (the x-t
 * slice of the depth at one image column, filled in frame by frame), from the tensors evaluation leaves on
 * the device straight to the bytes of the output file.  No atomics, no allocation, no synchronisation,
 * capturable in a graph; results stay on the device.  Argument checks run before any launch.
 *
 * vda_depth_absdiff_range: range [2] float (DEVICE) = (min, max) over the n >= 1 elements of
 *   e = valid ? fabsf(b - a) : 0.0f          (a = pred, b = gt: the subtraction is gt - pred, one fp32 operation)
 *   which is the error map as displayed, zeros included (vis_util.py:84-94 over utils/metrics.py:92-98).
 *   valid (uint8, non-zero = valid) may be NULL.  The reduction of vda_depth_range: block partials in ws, then
 *   one block; NaNs are skipped; a and b need 4-byte alignment only.  ws: vda_depth_absdiff_range_workspace(n)
 *   bytes of device memory owned by the caller, 4-byte aligned, no initialisation, nothing kept between calls.
 *
 * vda_panel_compose: for the F output frames t = t0 .. t0 + F - 1 of a scene of N frames, out holds frame
 *   after frame a canvas of rows * H x cols * W pixels in `layout` (VDA_VIS_HWC, VDA_VIS_PLANAR444 or
 *   VDA_VIS_PLANAR420 of vda_depth_colorize, with the canvas as the frame);
 *   vda_panel_compose_bytes(F, rows, cols, H, W, layout) bytes, nothing is written outside them.
 *   tiles: ntiles <= 12 descriptors in HOST memory (they travel in the kernel arguments), each in its own grid
 *   cell (row < rows <= 4, col < cols <= 3).  A tile with frame offset o >= 0 and `frames` source frames shows
 *   source frame s = t - o at canvas frame t; all its operands are indexed by s.  Per canvas pixel (y, px) of a
 *   tile, with S = H * W:
 *     VDA_TILE_RGB    a = uint8 [frames, H, W, 3] (any alignment): the pixel itself.  In VDA_VIS_HWC a copy; in
 *                     the planar layouts BT.601 limited range in fp32, every operation rounded once, no
 *                     contraction, the constants rounded to fp32 first:
 *                       y = (0.299 r + 0.587 g) + 0.114 b;  u = (b - y) / 1.772;  v = (r - y) / 1.402
 *                       Y = q(y * (219 / 255) + 16);  U = q(u * (224 / 255) + 128);  V likewise
 *                       q(x) = clamp(rintf(x), 0, 255)          (ties to even; IEEE division)
 *                     Outside 0 <= s < frames the pixel is black.
 *     VDA_TILE_DEPTH  a = float [frames, H, W]: v = a[s, y, px], or 0.0f outside 0 <= s < frames (a warmed-up
 *                     method before its first frame, vis_util.py:148-151), then lut[tile.lut][i] with the
 *                     index rule of vda_depth_colorize over tile.range (DEVICE [2] float):
 *                       x = (v - range[0]) / (range[1] - range[0]) * 255.0f;  i = (uint8_t)x by truncation,
 *                       NaN or x <= 0 -> 0, x >= 255 -> 255
 *     VDA_TILE_ERROR  a = pred, b = gt float [frames, H, W], valid uint8 [frames, H, W] or NULL:
 *                     v = valid ? fabsf(b - a) : 0.0f, or 0.0f outside 0 <= s < frames, then as VDA_TILE_DEPTH
 *     VDA_TILE_XT     a = float [frames, H, W], the whole video: the stability image [H, N] stretched to the
 *                     tile's width, never materialised:  c = (px * N) / W in 64-bit integers, s = c - o,
 *                     v = (c <= t && 0 <= s < frames) ? a[s, y, xstar] : 0.0f, then as VDA_TILE_DEPTH
 *   A cell without a tile is black.  Black is RGB (0, 0, 0): bytes (16, 128, 128) in the planar layouts.
 *   lut0 / lut1: the at most two distinct [256, 3] uint8 tables (DEVICE, any alignment) the tiles name, staged
 *   once per block in LDS; as in vda_depth_colorize the kernel does not know their colour space: RGB rows for
 *   VDA_VIS_HWC, converted YUV rows for the planar layouts.  4:2:0 chroma is (a + b + c + d + 2) >> 2 over 2x2
 *   blocks of the canvas's converted samples, the last row / column of the canvas repeated at odd sizes: a
 *   block straddles two tiles when H or W is odd.
 *   Float operands 4-byte aligned, out any address (dword stores around bytewise heads and tails).
 *   1 <= F <= 65535, 0 <= t0, t0 + F <= N, 0 <= xstar < W, rows * H * cols * W < 2^31.
 *   vda_tile_size() is sizeof(vda_tile): a binding checks its mirror against it.
 *   Deviations from the reference's matplotlib figure:
 *     colour index: imshow bins a value as min(int(x * 256), 255) after Normalize; the panels use the index rule
 *       above (* 255, truncation), so that one rule serves every depth picture the project writes.  The end
 *       colours for out-of-range values are the same.
 *     frame pairing: the reference's plot shows a warmed-up method one frame late against the GT it is
 *       subtracted from (vis_util.py:148, :157-164 index t - t_warmup with t_warmup = o), while its logged
 *       numbers pair gt[o + k] with pred[k] (calculate_metrics.py:223-226).  The panels follow the numbers.
 *     axes and text: no axes, titles, legend or line plot; tiles abut.
 */
enum {
  VDA_TILE_RGB = 0,
  VDA_TILE_DEPTH = 1,
  VDA_TILE_ERROR = 2,
  VDA_TILE_XT = 3
};
typedef struct vda_tile {
  int32_t kind;          /* VDA_TILE_* */
  int32_t row, col;      /* the grid cell */
  int32_t offset;        /* o: canvas frame t shows source frame t - o */
  int32_t frames;        /* source frames */
  int32_t lut;           /* 0 or 1: lut0 / lut1 (not RGB) */
  const void* a;         /* RGB: uint8 frames; DEPTH, XT: float depth; ERROR: pred */
  const float* b;        /* ERROR: gt */
  const uint8_t* valid;  /* ERROR: mask or NULL */
  const float* range;    /* DEVICE [2] (min, max) (not RGB) */
} vda_tile;
int64_t vda_tile_size(void);
int64_t vda_depth_absdiff_range_workspace(int64_t n);
int vda_depth_absdiff_range(const float* a, const float* b, const uint8_t* valid, int64_t n, float* range, void* ws,
                            int64_t ws_bytes, void* stream);
int64_t vda_panel_compose_bytes(int32_t F, int32_t rows, int32_t cols, int32_t H, int32_t W, int32_t layout);
int vda_panel_compose(const vda_tile* tiles, int32_t ntiles, int32_t rows, int32_t cols, int32_t F, int32_t t0,
                      int32_t N, int32_t H, int32_t W, int32_t xstar, const uint8_t* lut0, const uint8_t* lut1,
                      int32_t layout, uint8_t* out, void* stream);

/*
 * Planar YUV frames, as a YUV4MPEG2 (.y4m) file holds them, to RGB and to the network input, so that a video
 * is uploaded as the bytes of its file (1.5 B per pixel at 4:2:0) and never decoded on the host.  No atomics, no
 * allocation, no synchronisation, capturable in a graph.
 *
 * Source: src holds N frames, frame n at src + n * frame_stride bytes (frame_stride >= the payload size below,
 * so frames may be padded).  Within a frame the Y plane (h * w bytes) comes first, then U, then V, ch * cw
 * bytes each:
 *   VDA_YUV_420   cw = (w+1)/2, ch = (h+1)/2      VDA_YUV_422   cw = (w+1)/2, ch = h
 *   VDA_YUV_444   cw = w, ch = h                  VDA_YUV_MONO  no chroma planes, u = v = 128
 * src (DEVICE) may have any byte alignment; wider loads are used only where an address allows them.
 *
 * vda_yuv_to_rgb: out uint8 [N, h, w, 3] (any alignment).  Chroma is taken nearest, u[y >> sy][x >> sx], then
 *   BT.601 limited range -> RGB in fp32, every operation rounded once, no contraction:
 *     yf = (y - 16) * float(255.0 / 219.0);  uf = (u - 128) * float(255.0 / 224.0);  vf likewise
 *     r = yf + 1.402f * vf;  g = (yf - 0.344136f * uf) - 0.714136f * vf;  b = yf + 1.772f * uf
 *   then rintf (ties to even), clamp to 0..255, cast: the bits numpy float32 gives.  h, N <= 65535 (the grid).
 *
 * vda_preprocess_yuv: out float [N, 3, H, W] = vda_preprocess_frames applied to the RGB frames above, bit for
 *   bit (both kernels instantiate one device function).  Two routes, chosen from (h, w, H, W) alone: a
 *   workgroup converts the source footprint of its tile of output pixels once into LDS and interpolates from
 *   there; when a strong downscale makes that footprint exceed the compiled capacity, vda_yuv_to_rgb into ws
 *   followed by the RGB kernel.  ws: vda_preprocess_yuv_workspace(N, h, w, H, W) bytes of device memory owned
 *   by the caller, 0 when the tile route serves the shape (ws may be NULL then); it needs no initialisation.
 *   H, N <= 65535; on the workspace route also h <= 65535.
 *
 * vda_yuv_downscale: out uint8 [N, h2, w2, 3] (any alignment) = the RGB frames of vda_yuv_to_rgb resized as
 *   Pillow's Image.resize((w2, h2), Image.BICUBIC) resizes an 8-bit image (what read_video_frames does for
 *   --max_res), bit for bit.  That resampler is separable and runs in integer fixed point; per axis, for input
 *   size `in` and output size `out`, in IEEE doubles with one rounding per operation:
 *     scale = in / out;  fs = max(scale, 1);  support = 2 * fs;  ksize = (int)ceil(support) * 2 + 1
 *     for xx < out:  center = (xx + 0.5) * scale
 *       xmin = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - xmin
 *       w[x] = bicubic((x + xmin - center + 0.5) * (1 / fs)) for x < n, summed in that order into ww; w[x] /= ww
 *       k[xx][x] = (int)(w[x] * 2^22 + (w[x] < 0 ? -0.5 : 0.5));  k[xx][n ..] = 0;  bounds[xx] = (xmin, n)
 *     bicubic(x), a = -0.5:  |x| < 1: ((a + 2)|x| - (a + 3)) x^2 + 1;  |x| < 2: (((|x| - 5)|x| + 8)|x| - 4) a;  else 0
 *     pixel = clamp((2^21 + sum_x src[xmin + x] * k[xx][x]) >> 22, 0, 255)      (int32, arithmetic shift)
 *   The horizontal pass runs first over the three channels and is rounded to uint8, then the vertical pass; a
 *   pass whose size does not change (w2 == w, h2 == h) copies, and its tables are not read (they may be NULL).
 *   An axis may also grow (ensure_even adds a pixel): the tables carry it.
 *   vda_resample_taps(in, out) = ksize and vda_resample_tables fill k [out, ksize] and bounds [out, 2] on the
 *   HOST: pure functions, no device, no allocation, no state.  vda_yuv_downscale takes the tables of the two
 *   axes in DEVICE memory: kx [w2, vda_resample_taps(w, w2)], bx [w2, 2], ky [h2, vda_resample_taps(h, h2)],
 *   by [h2, 2], int32, 4-byte aligned.  Table entries are clamped to the staged footprint, so wrong tables
 *   give wrong pixels, never an access outside src or out.  The kernel multiplies with 24-bit multiplies: a
 *   coefficient must lie in [-2^23, 2^23), as every coefficient of vda_resample_tables does (a row's positive
 *   coefficients sum to at most 1.13 * 2^22 over every ratio from 5 -> 6 to 10240 -> 1280).
 *   One route: a workgroup owns 64 x 16 output pixels of a frame, converts the source rows it needs 8 at a time
 *   into LDS, filters them horizontally into LDS as uint8, filters that vertically and stores each row of the
 *   tile as a bytewise head, dwords and a bytewise tail.  Neither the RGB frame nor the intermediate is written
 *   to memory; vda_yuv_downscale_workspace is 0 for every shape and ws may be NULL.
 *   Compiled cap: at most 29 coefficients per axis (a ratio in / out up to 7, e.g. 8960 -> 1280) and at most
 *   64 KiB of LDS for the tile.  vda_yuv_downscale_ok(h, w, h2, w2) is 1 when the kernel serves the shape;
 *   otherwise vda_yuv_downscale returns -22 without launching (callers then resize on the host).
 *   h2, N <= 65535.
 */
enum {
  VDA_YUV_420 = 0,
  VDA_YUV_422 = 1,
  VDA_YUV_444 = 2,
  VDA_YUV_MONO = 3
};
int vda_yuv_to_rgb(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride, int32_t chroma,
                   uint8_t* out, void* stream);
int64_t vda_preprocess_yuv_workspace(int32_t N, int32_t h, int32_t w, int32_t H, int32_t W);
int vda_preprocess_yuv(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride, int32_t chroma,
                       float* out, int32_t H, int32_t W, const float* mean, const float* stdv, void* ws,
                       int64_t ws_bytes, void* stream);
int32_t vda_resample_taps(int32_t in, int32_t out);
int vda_resample_tables(int32_t in, int32_t out, int32_t* k, int32_t* bounds);
int vda_yuv_downscale_ok(int32_t h, int32_t w, int32_t h2, int32_t w2);
int64_t vda_yuv_downscale_workspace(int32_t N, int32_t h, int32_t w, int32_t h2, int32_t w2);
int vda_yuv_downscale(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride, int32_t chroma,
                      const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by, uint8_t* out,
                      int32_t h2, int32_t w2, void* ws, int64_t ws_bytes, void* stream);

/*
 * fp32 mode (infer_video_depth(fp32=True) / autocast off, video_depth.py:366-368): the same ops
 * with fp32 activations AND fp32 weights, fp32 accumulation on the exact-f32 MFMA
 * (v_mfma_f32_16x16x4_f32), exact-erf GELU, expf softmax.  Same layouts and epilogue contract as
 * the fp16 entry points above (vda_epilogue.res / res2 are float here).  Parity tier (i) of
 * SURVEY.md §8(d).  Requirements: K, ldx, N multiples of 4 (GEGLU / SwiGLU: N % 32 == 0); conv Cin, Cout
 * multiples of 4; spatial attention D == 64; temporal attention T <= 32, even D <= 192.
 * vda_gemm_f32 and vda_conv2d_f32 return -22 before any launch for what their kernel does not
 * implement or cannot address (every row access is a float4):
 *   ldx < K; ldy, ldres or ldres2 not a multiple of 4 (res / res2 rows may be strided otherwise);
 *   drop_period != 0 (vda_gemm only: the fp32 kernel stores all M rows);
 *   ln_stats, stats_out, res2_h / res2_w (fp16 entry points only);
 *   a rowbias with rdiv <= 0 or rmod <= 0;
 *   GEMM: VDA_ACT_GEGLU / VDA_ACT_SWIGLU together with a rowbias, a res2 or the pixel-shuffle store (as
 *   vda_gemm); conv: VDA_ACT_GEGLU / VDA_ACT_SWIGLU, the pixel-shuffle store.
 * sched is ignored (no persistent fp32 kernel).
 */
int vda_gemm_f32(const float* x, int64_t ldx, const float* w, float* y, int64_t ldy,
                 int32_t M, int32_t N, int32_t K, const vda_epilogue* epi, void* stream);
int vda_conv2d_f32(const float* x, const float* w, float* y, int32_t BT, int32_t H, int32_t W,
                   int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t pad,
                   int32_t pre_relu, const vda_epilogue* epi, void* stream);
int vda_layernorm_f32(const float* x, int64_t ldx, float* y, const float* gamma, const float* beta,
                      int32_t rows, int32_t C, float eps, int32_t skip_period, void* stream);
int vda_groupnorm_f32(const float* x, float* y, const float* gamma, const float* beta, int32_t F,
                      int32_t S, int32_t C, int32_t groups, float eps, void* stream);
int vda_spatial_attention_f32(const float* qkv, float* out, int32_t B, int32_t N, int32_t H,
                              int32_t D, float scale, void* stream);
int vda_temporal_attention_f32(const float* qkv, float* out, int32_t B, int32_t T, int32_t S,
                               int32_t H, int32_t D, float scale, float rope_theta, void* stream);
int vda_upsample_bilinear_f32(const float* x, float* y, int32_t BT, int32_t H, int32_t W, int32_t C,
                              int32_t Ho, int32_t Wo, void* stream);
int vda_patch_im2col_f32(const float* img, float* a, int32_t BT, int32_t H, int32_t W, int32_t Kp,
                         void* stream);
/* Depth tail in fp32: bilinear resize into ws_up [BT, Ho, Wo, C], conv3x3(C -> 32, w1 [32, 3, 3, C],
 * +b1) -> ReLU into ws_mid [BT*Ho*Wo, 32], then 1x1 (w2 [32], +b2) -> ReLU -> depth [BT, Ho, Wo]. */
int vda_depth_head_f32(const float* x, const float* w1, const float* b1, const float* w2,
                       const float* b2, float* depth, float* ws_up, float* ws_mid, int32_t BT,
                       int32_t Hin, int32_t Win, int32_t C, int32_t Ho, int32_t Wo, void* stream);

/* The tuning entry points (vda_debug_*) exist only in the tuning build of the library
 * (make tune -> build/tune/libvda.so): include/vda_tune.h.  This library keeps no mutable global
 * state; its kernel routes are the automatic ones. */

#ifdef __cplusplus
}
#endif
#endif /* VDA_H */
