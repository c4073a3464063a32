// MFMA GEMM + implicit-GEMM convolution with fused epilogues (gfx950): route decision and launch.
//
// Y[m, n] = epi( sum_k X[m, k] * W[n, k] ) for every nn.Linear, 1x1 conv, ConvTranspose2d(k=s) and the
// 3x3 convs that no dedicated conv kernel serves (see include/vda.h for the reference call sites).
// Three kernel families, all instantiated by this one translation unit:
//   vda_gemm_tile.h    gemm_reg_kernel (4 waves, register-staged; the conv with a bilinear-resize loader)
//                      and gemm_kernel (LDS-DMA pipeline, one tile per block, BM x BN from 64x64 to 256x256)
//   vda_gemm_phased.h  gemm256_tile / gemm256_kernel (8 waves, 4-phase K steps, persistent for dense GEMMs;
//                      register and LDS-staged epilogues), the route of every large shape
// Which kernel serves a call is decided in ONE place, gemm_route: the tile configuration, for the phased
// kernels the instantiation, and whether that kernel writes epi.stats_out itself.  launch() runs what the
// route says; vda_gemm / vda_gemm_check ask the same route whether the call gets the one kernel that
// implements drop_period or the LN fold with a row bias; the conv router asks vda_gemm_phased256_serves
// before it builds an im2col matrix for the dense kernel.  A kernel is instantiated here only if the
// automatic route can name it or a test launches it through the tuning build's vda_debug_force_tile.
// Besides the route: the knobs, the epilogue argument checks and the launch functions of vda_internal.h
// through which the conv router (vda_conv2d.hip) and the depth-head router (vda_depth_head.hip) reach the
// kernels.
#include "vda_gemm_tile.h"
#include "vda_gemm_phased.h"
#include <algorithm>

// Knobs of the tuning build (include/vda_tune.h); compile-time constants in the product library.
VDA_KNOB_DEF(int, g_force_tile, -1);  // vda_debug_force_tile (declared in vda_internal.h)

// The phased kernels' dense operand path: K in whole 64-column steps and 32-bit buffer offsets over X and W.
static bool phased_dense_ok(long M, long N, long K, long ldx) {
  return K % 64 == 0 && M * ldx * 2 < (1L << 31) && N * K * 2 < (1L << 31);
}

bool vda_gemm_phased256_serves(long M, long N, long K, long ldx) {
  return N >= 256 && M >= 4096 && phased_dense_ok(M, N, K, ldx);
}

namespace {

VDA_KNOB(int, g_persist, -1);    // vda_debug_gemm_sched; -1 = automatic

// The gemm256_kernel<XR, WR, CONV, ACT, ROWB, LNF, EK> instantiation a route names (cfg 4 / 5)
enum Phased {
  PH_STAGED,    // <.., false, false, 0>: the general LDS-staged epilogue
  PH_ROWB,      // <.., true>:            the same with a per-row bias
  PH_REG,       // <.., false, false, 1>: bias (+ GELU) from registers
  PH_LNF,       // <.., false, true, 0>:  LN fold, staged
  PH_LNF_REG,   // <.., false, true, 1>:  LN fold + bias (+ GELU) from registers; the only epilogue that drops rows
  PH_LNF_ROWB,  // <.., false, true, 3>:  LN fold + per-frame row bias (motion-module q/k/v)
};

struct GemmRoute {
  int cfg;            // tile configuration: the cases of launch_cfg
  Phased phased;      // cfg 4 / 5
  bool writes_stats;  // the kernel's own epilogue serves epi.stats_out (else: vda_row_partials_launch after it)
};

// Pure function of the call, the tuning build's g_force_tile and the CU count.  Looks at sizes, at whether
// each epilogue pointer is set and at alignments; never at what a pointer points to.
GemmRoute gemm_route(const GemmParams& p, bool conv) {
  const vda_epilogue& e = p.epi;
  const bool plain = e.act == VDA_ACT_NONE, gelu = e.act == VDA_ACT_GELU;
  const bool geglu = vda_glu(e.act);  // GEGLU and SwiGLU take the same routes: they differ in the gate alone
  GemmRoute r{g_force_tile, PH_STAGED, false};
  if (r.cfg < 0) {
    // measured on MI355X (tools/archive/bench_gemm.py): 256x256 wins every large-N shape; N = 128 prefers
    // 256x128; short K (<= 256) and narrow N prefer the 2-blocks-per-CU 128x64 tile.
    const bool a16 = ((uintptr_t)p.y % 16 == 0) && p.ldy % 8 == 0 && p.N % 8 == 0 &&
                     (!e.res || ((uintptr_t)e.res % 16 == 0 && e.ldres % 8 == 0)) &&
                     (!e.res2 || ((uintptr_t)e.res2 % 16 == 0 && e.ldres2 % 8 == 0)) &&
                     (!geglu || (p.N / 2) % 8 == 0);
    // per-row bias only in the dense, activation-free phased instantiation
    const bool rowb_ok = !e.rowbias || (!conv && plain);
    const bool ph256 = (conv ? p.N >= 256 && p.M >= 4096 : vda_gemm_phased256_serves(p.M, p.N, p.K, p.ldx)) &&
                       rowb_ok && (e.store != VDA_STORE_ROWS || a16);
    const bool ph512 = p.N == 128 && p.M >= 8192 && (conv || phased_dense_ok(p.M, p.N, p.K, p.ldx)) && rowb_ok &&
                       a16 && e.store == VDA_STORE_ROWS && !e.ln_stats;
    if (p.N <= 64 || (p.K <= 256 && p.N < 256)) r.cfg = 2;
    else if (ph256) r.cfg = 4;
    else if (ph512) r.cfg = 5;
    else if (p.N >= 256 && p.M >= 4096) r.cfg = 3;
    else if (p.N >= 128 && p.M >= 4096) r.cfg = 1;
    else if (conv) r.cfg = 0;
    else {
      // small M (the streaming mode's one-frame encoder, M = 1,370): the largest tile that still
      // gives >= 2 tiles per CU, else 64x64 (tools/archive/bench_gemm_small.py: ViT-L fc2 72.8 -> 43.5 us,
      // proj 24.0 -> 14.0, qkv 29.5 -> 25.0, fc1 34.2 -> 30.3)
      const long ncu2 = 2L * vda_cu_count();
      auto ntiles = [&](int bm, int bn) { return (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
      r.cfg = ntiles(128, 128) >= ncu2 ? 0 : ntiles(128, 64) >= ncu2 ? 2 : 6;
    }
  }
  if (!conv && (r.cfg == 4 || r.cfg == 5)) {  // the convs run the staged epilogue only
    const bool xr2 = r.cfg == 4;  // every epilogue but the staged and the row-bias one is 256x256 only
    // what the register epilogues implement: bias (+ GELU) and a plain row store, nothing else
    const bool reg = e.store == VDA_STORE_ROWS && e.bias && !e.gamma && !e.res && !e.res2 && !e.rowbias && !e.stats_out;
    if (plain && e.rowbias) {
      r.phased = xr2 && e.ln_stats ? PH_LNF_ROWB : PH_ROWB;
    } else if (xr2 && e.ln_stats && (plain || gelu || geglu)) {
      r.phased = reg && !geglu ? PH_LNF_REG : PH_LNF;
    } else if (xr2 && reg && (plain || gelu)) {
      r.phased = PH_REG;
    } else {
      // gemm256_tile's store_with_stats: the dense activation-free 256x256 staged epilogue with at most one
      // residual forms the row partials from the values it stores
      r.writes_stats = xr2 && plain && !(e.res && e.res2);
    }
  }
  return r;
}

// grid of a phased launch (see gemm256_kernel).  Every block starts at once.  Two start delays were
// measured and dropped: half of the blocks half a tile late when the last round is short (+0.4 % with
// one clip in flight, -0.6 % with the two clips the drivers run: the sleeping blocks hold CUs the other
// clip's kernels would use), and every block a fraction of a tile late to spread the CUs' epilogue store
// bursts (within +-3 % on all four encoder shapes, no gain); docs/HISTORY.md.
int phased_sched(int ntiles, bool conv) {
  // measured in situ: persistent pays for the dense GEMMs, one block per tile for the convs
  const int persist = conv ? 0 : (g_persist >= 0 ? g_persist : vda_cu_count());
  return persist == 0 ? ntiles : std::min(ntiles, persist);
}

template <int BM, int BN, int NWM, int NWN, int KB, int NS, bool CONV, int ACT>
void launch_tile(const GemmParams& p, hipStream_t st) {
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_kernel<BM, BN, NWM, NWN, KB, NS, CONV, ACT>), dim3(tiles_m * tiles_n), dim3(NWM * NWN * 64),
                     0, st, p, tiles_m, tiles_n);
}

// Launches the instantiation `v` names.  The if constexpr lines are the list of what is built: gemm_route
// names nothing else for this (XR, CONV, ACT).
template <int XR, int WR, bool CONV, int ACT>
void launch_phased(Phased v, const GemmParams& p, hipStream_t st) {
  const int BM = 128 * XR, BN = 128 * WR;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int grid = phased_sched(tiles_m * tiles_n, CONV);
  auto go = [&](void (*kernel)(GemmParams, int, int)) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), 0, st, p, tiles_m, tiles_n);
  };
  constexpr bool PLAIN = ACT == VDA_ACT_NONE, GELU = ACT == VDA_ACT_GELU, GEGLU = vda_glu(ACT);
  constexpr bool D256 = !CONV && XR == 2;
  if constexpr (!CONV && PLAIN)
    if (v == PH_ROWB) return go(gemm256_kernel<XR, WR, CONV, ACT, true>);
  if constexpr (D256 && PLAIN)
    if (v == PH_LNF_ROWB) return go(gemm256_kernel<XR, WR, CONV, ACT, false, true, 3>);
  if constexpr (D256 && (PLAIN || GELU || GEGLU))
    if (v == PH_LNF) return go(gemm256_kernel<XR, WR, CONV, ACT, false, true>);
  if constexpr (D256 && (PLAIN || GELU)) {
    if (v == PH_LNF_REG) return go(gemm256_kernel<XR, WR, CONV, ACT, false, true, 1>);
    if (v == PH_REG) return go(gemm256_kernel<XR, WR, CONV, ACT, false, false, 1>);
  }
  go(gemm256_kernel<XR, WR, CONV, ACT, false>);  // PH_STAGED
}

template <bool CONV, int ACT>
int launch_cfg(const GemmRoute& r, const GemmParams& p, hipStream_t st) {
  switch (r.cfg) {
    case 1: launch_tile<256, 128, 4, 2, 32, 4, CONV, ACT>(p, st); break;
    case 2: launch_tile<128, 64, 2, 2, 32, 4, CONV, ACT>(p, st); break;
    case 3: launch_tile<256, 256, 2, 4, 32, 4, CONV, ACT>(p, st); break;
    case 4: launch_phased<2, 2, CONV, ACT>(r.phased, p, st); break;
    case 5: launch_phased<4, 1, CONV, ACT>(r.phased, p, st); break;
    case 6:
    case 7:  // 64-row tiles: the dense small-M choice and the tuning build's dense tests; no conv reaches them
      if constexpr (CONV) {
        return vda_set_error(-22, "conv: no 64-row tile configuration (6 / 7)");
      } else {
        if (r.cfg == 6) launch_tile<64, 64, 2, 2, 32, 4, CONV, ACT>(p, st);
        else launch_tile<64, 128, 2, 2, 32, 4, CONV, ACT>(p, st);
      }
      break;
    default: launch_tile<128, 128, 2, 2, 32, 4, CONV, ACT>(p, st); break;
  }
  return 0;
}

template <bool CONV>
int launch(const GemmParams& p, hipStream_t st) {
  const GemmRoute r = gemm_route(p, CONV);
  int rc = 0;
  switch (p.epi.act) {
    case VDA_ACT_GELU:
    case VDA_ACT_GEGLU:
    case VDA_ACT_SWIGLU:  // vda_conv2d admits none / ReLU only: no conv kernel is built for these
      if constexpr (CONV) return vda_set_error(-22, "conv epilogue: activation none / relu");
      else rc = p.epi.act == VDA_ACT_GELU    ? launch_cfg<CONV, VDA_ACT_GELU>(r, p, st)
                : p.epi.act == VDA_ACT_GEGLU ? launch_cfg<CONV, VDA_ACT_GEGLU>(r, p, st)
                                             : launch_cfg<CONV, VDA_ACT_SWIGLU>(r, p, st);
      break;
    case VDA_ACT_RELU: rc = launch_cfg<CONV, VDA_ACT_RELU>(r, p, st); break;
    default: rc = launch_cfg<CONV, VDA_ACT_NONE>(r, p, st); break;
  }
  if (rc) return rc;
  VDA_LAUNCH_CHECK();
  if (p.epi.stats_out && !r.writes_stats) return vda_row_partials_launch(p.y, p.ldy, p.epi.stats_out, p.M, p.N, st);
  return 0;
}

// vda_gemm's argument and route checks; fills p for the launch
int gemm_check(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int32_t M, int32_t N, int32_t K,
               const vda_epilogue* epi, GemmParams& p) {
  VDA_CHECK_ARG(x && w && y, "null pointer");
  VDA_CHECK_ARG(M > 0 && N > 0 && K > 0, "empty GEMM");
  VDA_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0 && ldx >= K, "K and ldx must be multiples of 8, ldx >= K");
  VDA_CHECK_ARG(N % 4 == 0 && ldy % 4 == 0, "N and ldy must be multiples of 4");
  p = GemmParams{};
  p.x = (const h16*)x; p.ldx = ldx; p.w = (const h16*)w; p.y = (h16*)y; p.ldy = ldy;
  p.M = M; p.N = N; p.K = K;
  p.epi = epi ? *epi : vda_default_epi();
  if (p.epi.rdiv <= 0) p.epi.rdiv = 1;
  if (p.epi.rmod <= 0) p.epi.rmod = 1;
  const vda_epilogue& e = p.epi;
  VDA_CHECK_ARG(e.res2_h == 0 && e.res2_w == 0, "upsampled res2: vda_conv2d only");
  VDA_CHECK_ARG(!e.bias9, "bias9: vda_conv2d only");
  // Two epilogue options exist in one kernel each, so the call must be one the automatic route gives to
  // that kernel (any other kernel would store all M rows, or ignore the row bias); what is left here are
  // those kernels' own preconditions.
  const GemmRoute r = gemm_route(p, false);
  const bool auto256 = g_force_tile < 0 && r.cfg == 4;
  if (e.drop_period != 0) {  // only the phased route's register LN-fold epilogue (EK 1) drops rows
    VDA_CHECK_ARG(auto256 && r.phased == PH_LNF_REG && e.act == VDA_ACT_NONE && e.ln_colsum && e.drop_period >= 256 &&
                      N % 256 == 0,
                  "drop_period: >= 256, with ln_stats + bias, no activation / gamma / res / rowbias / stats_out, "
                  "N % 256 == 0, M >= 4096, K % 64 == 0, 16-byte aligned rows");
  }
  int rc = vda_check_epi(e, M, N);
  if (rc) return rc;
  if (e.ln_stats && e.rowbias) {  // only the phased 256x256 route (EK 3) implements the pair
    VDA_CHECK_ARG(auto256 && r.phased == PH_LNF_ROWB && N % 256 == 0 && (uintptr_t)x % 16 == 0,
                  "ln_stats with rowbias needs N % 256 == 0, M >= 4096, K % 64 == 0, 16-B aligned rows");
  }
  return 0;
}

}  // namespace

// ---- the launch functions of vda_internal.h ----
int vda_launch_conv_reg(const GemmParams& p, hipStream_t st) {
  const int tiles_m = (p.M + 127) / 128;
  if (p.N >= 128) {
    const int tiles_n = (p.N + 127) / 128;
    if (p.epi.act == VDA_ACT_RELU)
      hipLaunchKernelGGL((gemm_reg_kernel<128, 128, ConvLoader, VDA_ACT_RELU>), dim3(tiles_m * tiles_n), dim3(256), 0, st, p, tiles_n);
    else
      hipLaunchKernelGGL((gemm_reg_kernel<128, 128, ConvLoader, VDA_ACT_NONE>), dim3(tiles_m * tiles_n), dim3(256), 0, st, p, tiles_n);
  } else {
    const int tiles_n = (p.N + 63) / 64;
    if (p.epi.act == VDA_ACT_RELU)
      hipLaunchKernelGGL((gemm_reg_kernel<128, 64, ConvLoader, VDA_ACT_RELU>), dim3(tiles_m * tiles_n), dim3(256), 0, st, p, tiles_n);
    else
      hipLaunchKernelGGL((gemm_reg_kernel<128, 64, ConvLoader, VDA_ACT_NONE>), dim3(tiles_m * tiles_n), dim3(256), 0, st, p, tiles_n);
  }
  VDA_LAUNCH_CHECK();
  return 0;
}

vda_epilogue vda_default_epi() {
  vda_epilogue e{};
  e.rdiv = 1; e.rmod = 1;
  return e;
}

int vda_check_epi(const vda_epilogue& e, int M, int N) {
  VDA_CHECK_ARG(!e.rowbias || (e.rdiv > 0 && e.rmod > 0), "rowbias needs rdiv, rmod > 0");
  VDA_CHECK_ARG(e.act >= 0 && e.act <= 4, "unknown activation");
  VDA_CHECK_ARG(!vda_glu(e.act) || (N % 32 == 0 && !e.rowbias && e.store == 0 && !e.res2),
                "GEGLU needs N % 32 == 0, no rowbias/res2, row store");
  VDA_CHECK_ARG(e.store == VDA_STORE_ROWS ||
                (e.store == VDA_STORE_PIXEL_SHUFFLE && e.ps_k > 0 && e.ps_cout > 0 && e.ps_cout % 4 == 0 &&
                 e.ps_hin > 0 && e.ps_win > 0 && N == e.ps_k * e.ps_k * e.ps_cout && !e.res && !e.res2),
                "bad pixel-shuffle store geometry");
  // the LN fold exists for the activation-free, GELU, GEGLU and SwiGLU epilogues (every kernel route applies it
  // there; anything else would silently run an un-normalised GEMM); with a row bias only on the
  // phased route's EK 3 epilogue (vda_gemm checks the route)
  VDA_CHECK_ARG(!e.ln_stats || (e.ln_colsum && e.store == VDA_STORE_ROWS && !e.gamma &&
                                 (e.act == VDA_ACT_NONE || e.act == VDA_ACT_GELU || vda_glu(e.act))),
                "ln_stats needs ln_colsum, a row store, no gamma, activation none / gelu / geglu");
  VDA_CHECK_ARG(!e.ln_stats || !e.rowbias ||
                    (e.act == VDA_ACT_NONE && e.bias && !e.res && !e.res2 && !e.stats_out && e.rdiv >= 256),
                "ln_stats with rowbias needs a bias, no activation / residual / stats_out, rdiv >= 256");
  VDA_CHECK_ARG(!e.ln_stats || (e.ln_parts >= 0 && e.ln_parts <= 4), "ln_parts must be 0 .. 4");
  // the phased route stages the statistics in 16-byte pieces, reading the last one 8 B early when the
  // float count is not a multiple of 4: the buffer must hold at least one whole piece (M * P >= 2)
  VDA_CHECK_ARG(!e.ln_stats || (long)M * (e.ln_parts > 0 ? e.ln_parts : 1) >= 2, "ln_stats needs M * max(ln_parts, 1) >= 2");
  VDA_CHECK_ARG(!e.stats_out || (e.store == VDA_STORE_ROWS && !vda_glu(e.act)),
                "stats_out needs a row store and no GEGLU");
  VDA_CHECK_ARG(!e.res || e.ldres % 4 == 0, "ldres % 4");
  VDA_CHECK_ARG(!e.res2 || e.ldres2 % 4 == 0, "ldres2 % 4");
  return 0;
}

int vda_launch_gemm(const GemmParams& p, hipStream_t st) { return launch<false>(p, st); }

extern "C" int vda_gemm_check(int64_t ldx, int64_t ldy, int32_t M, int32_t N, int32_t K, const vda_epilogue* epi) {
  GemmParams p;
  void* const aligned = (void*)16;  // stands for 16-byte aligned x / w / y; never dereferenced
  return gemm_check(aligned, ldx, aligned, aligned, ldy, M, N, K, epi, p);
}

extern "C" int vda_gemm(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int32_t M,
                        int32_t N, int32_t K, const vda_epilogue* epi, void* stream) {
  GemmParams p;
  const int rc = gemm_check(x, ldx, w, y, ldy, M, N, K, epi, p);
  return rc ? rc : vda_launch_gemm(p, (hipStream_t)stream);
}

int vda_launch_conv_gemm(const GemmParams& p, hipStream_t st) { return launch<true>(p, st); }

int vda_launch_subpixel_gemm(const GemmParams& p, hipStream_t st) {
  if (!phased_dense_ok(p.M, p.N, p.K, p.ldx) || p.N % 256 != 0 || p.N > 8 * 256)
    return vda_set_error(-22, "sub-pixel conv: K % 64 == 0, N = 256 phases (<= 8), operands below 2 GiB");
  const int tiles_m = (p.M + 255) / 256, tiles_n = p.N / 256;
  const int grid = phased_sched(tiles_m * tiles_n, false);
  hipLaunchKernelGGL((gemm256_kernel<2, 2, false, VDA_ACT_NONE, false, false, 0, true>), dim3(grid), dim3(512), 0, st, p,
                     tiles_m, tiles_n);
  VDA_LAUNCH_CHECK();
  return 0;
}

int vda_launch_depth_gemm(const GemmParams& p, hipStream_t st) {
  const int tiles_m = (p.M + 255) / 256;
  hipLaunchKernelGGL((gemm_kernel<256, 64, 8, 1, 64, 2, true, ACT_DEPTH>), dim3(tiles_m), dim3(512), 0, st, p, tiles_m, 1);
  VDA_LAUNCH_CHECK();
  return 0;
}

#ifdef VDA_TUNING
extern "C" int vda_debug_force_tile(int32_t cfg) {
  g_force_tile = cfg;
  return 0;
}

extern "C" int vda_debug_gemm_sched(int32_t persist_blocks) {
  g_persist = persist_blocks;
  return 0;
}
#endif
