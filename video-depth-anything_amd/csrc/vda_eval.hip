// Ground-truth evaluation on the device: the masked inverse-depth least-squares fit and the seven
// depth metrics of the reference's eval.py, as two streaming reductions over resident data.
//
// fit:     align_prediction's frame_align_lstsq (utils/align.py:151-160, :192-207): over the valid pixels
//          minimise S (c0 pred + c1 - 1/gt)^2, report scale = 1/c0, shift = -c1/c0.  The reference builds
//          an [n_valid, 2] matrix on the host and calls an SVD lstsq; here it is five fp64 sums and the
//          2x2 closed form.
// metrics: utils/align.py:210-216 (align, clip, invert, clip) + utils/metrics.py:91-192 (OutlierRatio x3,
//          SignedRelative, AbsoluteDifference, AbsoluteRelative, MeanSquared), ten full-size numpy passes
//          in the reference, in one pass: eight fp64 sums per frame.
//
// Both are streaming passes (vda_stream.h) per frame: 16-byte loads on pred and element-aligned vector
// loads on gt / valid, a small kernel adds a frame's partials in index order, then the frames are added in
// frame order.  No atomics, so the same input gives the same bits on every run.  Every frame has its own
// head / tail (frames start at f * S, S is not a multiple of 4 in general) and its own blocks (grid.y = f),
// and the number of blocks per frame depends on S alone: frame f of an [F, S] call is summed exactly as a
// single-frame call on it would be.  Every per-pixel operation is one correctly rounded fp32 operation
// (no rcp, no contraction), so the aligned map equals separate torch fp32 ops bit for bit.  Invalid
// pixels are selected out, never multiplied out: gt may be 0 or NaN there (1/0 = inf, inf * 0 = NaN).
// HBM-bound: 9 B per element read (8 B without valid), + 4 B written with the aligned map.
#include "vda_stream.h"
#include "../../include/vda.h"

namespace {

constexpr int kFitSums = 5;
constexpr int kMetricSums = 8;
constexpr int kPartStride = 8;  // doubles per block partial, for both kernels
// A block takes at least kItersPerBlock 16-byte groups per thread while the frame is large enough;
// at most kMaxBlocksPerFrame blocks share a frame.
constexpr int64_t kItersPerBlock = 4;
constexpr int64_t kMaxBlocksPerFrame = 512;
constexpr int kMaxFrames = 65535;  // grid.y

// Blocks per frame: a function of S alone (see the header comment).
int blocks_per_frame(int64_t S) { return stream_grid(S, kStreamGroup * kItersPerBlock, kMaxBlocksPerFrame); }

// a_00 = S p^2, a_01 = S p, a_11 = S 1, b_0 = S p t, b_1 = S t over valid pixels, t = 1 / gt in fp32.
// Branch-free: an invalid pixel's p and t are replaced by +0 before they reach a sum (a select, so a NaN
// or inf there goes nowhere), and adding +0 leaves an fp64 accumulator's bits as they are (it is never -0:
// it starts at +0).  The count a_11 is a per-thread integer, made the exact fp64 sum s[2] at the end.
__device__ __forceinline__ void fit_accumulate(double (&s)[kFitSums], int& cnt, float p, float g, bool valid) {
  const float t = 1.f / g;
  const double dp = (double)(valid ? p : 0.f), dt = (double)(valid ? t : 0.f);
  s[0] = fma(dp, dp, s[0]);  // the product of two fp32 values is exact in fp64
  s[1] += dp;
  cnt += valid ? 1 : 0;
  s[3] = fma(dp, dt, s[3]);
  s[4] += dt;
}

// utils/align.py:210-216 per pixel.  clip(x, lo, hi) as numpy and torch.clamp do it: NaN passes through.
__device__ __forceinline__ float align_metric_depth(float p, float scale, float shift, float max_depth) {
#pragma clang fp contract(off)
  const float c = p - shift;
  float a = c / scale;
  a = a < 0.f ? 0.f : (a > 1.f ? 1.f : a);
  a = a == 0.f ? 1e-4f : a;
  float d = 1.f / a;
  d = d < 0.f ? 0.f : (d > max_depth ? max_depth : d);
  return d;
}

// S d/g, S |d|, S |d|/g, S d^2 into s[4..7] and the count and the outliers at 1.25 / 1.25^2 / 1.25^3 into
// c[0..3], over valid pixels (d = p - g).  The counts are per-thread integers (a thread sees far fewer than
// 2^31 pixels) and become the exact fp64 sums s[0..3] before the wave reduction.  An invalid pixel is
// skipped by a branch: the select form of fit_accumulate measured slower here (166 against 152 us at
// 64 x 720 x 1280).
// |d| / g is |d / g| bit for bit (rounding to nearest is symmetric), which saves a division.  So does the
// outlier ratio: for p >= g > 0 the rounded p / g is >= 1 >= the rounded g / p, so max(p/g, g/p) is
// hi / lo with hi = the larger of the two; where that identity fails (g <= 0, a NaN) both forms compare
// false against every threshold or both are +inf, so the flags are the reference's in every case.
__device__ __forceinline__ void metric_accumulate(double (&s)[kMetricSums], int (&c)[4], float p, float g, bool valid) {
#pragma clang fp contract(off)
  if (!valid) return;
  const float d = p - g;
  const bool pge = p >= g;
  const float hi = pge ? p : g, lo = pge ? g : p;
  const float mx = hi / lo;
  const float rel = d / g;
  const float sq = d * d;
  c[0] += 1;
  c[1] += mx > 1.25f ? 1 : 0;
  c[2] += mx > 1.5625f ? 1 : 0;
  c[3] += mx > 1.953125f ? 1 : 0;
  s[4] += (double)rel;
  s[5] += (double)fabsf(d);
  s[6] += (double)fabsf(rel);
  s[7] += (double)sq;
}

// Frame f = blockIdx.y, block b = blockIdx.x of gridDim.x: the block's sums go to
// part[(f * gridDim.x + b) * kPartStride ..].  The split is that of the frame's pred.
// METRICS = false: the five fit sums.  METRICS = true: the eight metric sums, and with `aligned` the
// metric depth of every pixel, valid or not.
template <bool METRICS, bool MASK>
__global__ __launch_bounds__(kStreamBlock) void eval_partial_kernel(const float* __restrict__ pred,
                                                                    const float* __restrict__ gt,
                                                                    const uint8_t* __restrict__ valid, int64_t S,
                                                                    const float* __restrict__ ss, int ss_per_frame,
                                                                    float max_depth, float* __restrict__ aligned,
                                                                    double* __restrict__ part) {
  constexpr int K = METRICS ? kMetricSums : kFitSums;
  const int64_t f = blockIdx.y;
  const float* pf = pred + f * S;
  const float* gf = gt + f * S;
  const uint8_t* vf = MASK ? valid + f * S : nullptr;
  float* af = (METRICS && aligned) ? aligned + f * S : nullptr;
  const StreamSplit sp = stream_split_f32(pf, S);
  float scale = 1.f, shift = 0.f;
  if (METRICS) {
    const float* sf = ss + (ss_per_frame ? 2 * f : 0);
    scale = sf[0];
    shift = sf[1];
  }
  double s[K];
#pragma unroll
  for (int j = 0; j < K; ++j) s[j] = 0.;
  int c[4] = {0, 0, 0, 0};  // the counts: four for the metrics, c[0] alone for the fit

  stream_walk(
      S, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4 p = *reinterpret_cast<const f4*>(pf + o);
        const f4a4 g = *reinterpret_cast<const f4a4*>(gf + o);
        bool m[4] = {true, true, true, true};
        if (MASK) {
          const u8x4a1 mv = *reinterpret_cast<const u8x4a1*>(vf + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) m[j] = mv[j] != 0;
        }
        if constexpr (METRICS) {
          f4a4 d;
#pragma unroll
          for (int j = 0; j < 4; ++j) d[j] = align_metric_depth(p[j], scale, shift, max_depth);
          if (af) *reinterpret_cast<f4a4*>(af + o) = d;
#pragma unroll
          for (int j = 0; j < 4; ++j) metric_accumulate(s, c, d[j], g[j], m[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) fit_accumulate(s, c[0], p[j], g[j], m[j]);
        }
      },
      [&](int64_t e) {
        const bool m = MASK ? vf[e] != 0 : true;
        if constexpr (METRICS) {
          const float d = align_metric_depth(pf[e], scale, shift, max_depth);
          if (af) af[e] = d;
          metric_accumulate(s, c, d, gf[e], m);
        } else {
          fit_accumulate(s, c[0], pf[e], gf[e], m);
        }
      });
  if constexpr (METRICS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = (double)c[j];
  } else {
    s[2] = (double)c[0];
  }
  block_store_partial<K>(s, part + (f * gridDim.x + blockIdx.x) * kPartStride);
}

// One wave per frame adds the frame's partials; lanes 0..K-1 store out[f * K + j].
template <int K>
__global__ __launch_bounds__(64) void frame_reduce_kernel(const double* __restrict__ part, int nparts,
                                                          double* __restrict__ out) {
  const int64_t f = blockIdx.x;
  wave_add_partials<K>(part + f * nparts * kPartStride, nparts, kPartStride, [&](int j, double v) {
    if ((int)threadIdx.x == j) out[f * K + j] = v;
  });
}

// (c0, c1) of the 2x2 normal equations to scale = 1 / c0, shift = -c1 / c0, rounded once on the store.
// No valid pixel (det == 0 with a_11 == 0), det == 0 or c0 == 0 -> (inf, 0).
__device__ __forceinline__ void fit_solve(const double (&a)[kFitSums], float* __restrict__ ss) {
#pragma clang fp contract(off)
  double c0 = 0., c1 = 0.;
  double scale = __builtin_inf(), shift = 0.;
  if (solve_2x2(a, c0, c1) && c0 != 0.) {
    scale = 1. / c0;
    shift = -c1 / c0;
  }
  ss[0] = (float)scale;
  ss[1] = (float)shift;
}

// tot[j] = fs[0][j] + fs[1][j] + ... in frame order, for one wave: 64 frames at a time are staged in LDS
// with coalesced loads, then thread j adds its column serially.  fs [F, K]; tot: K doubles in LDS.
template <int K>
__device__ __forceinline__ void frame_order_total(const double* __restrict__ fs, int F, double* tot) {
  __shared__ double buf[64 * K];
  double t = 0.;
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int nf = F - f0 < 64 ? F - f0 : 64;
    for (int i = threadIdx.x; i < nf * K; i += 64) buf[i] = fs[(int64_t)f0 * K + i];
    __syncthreads();
    if (threadIdx.x < K) {
      for (int f = 0; f < nf; ++f) t += buf[f * K + threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x < K) tot[threadIdx.x] = t;
  __syncthreads();
}

// per_frame: thread g solves frame g's sums.  Otherwise block 0 adds the frames' sums in frame order and
// thread 0 solves.  fsum [F, 5]; sums [G, 5] or NULL; ss [G, 2].
__global__ __launch_bounds__(64) void fit_solve_kernel(const double* __restrict__ fsum, int F, int per_frame,
                                                       double* __restrict__ sums, float* __restrict__ ss) {
  if (per_frame) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= F) return;
    double a[kFitSums];
#pragma unroll
    for (int j = 0; j < kFitSums; ++j) a[j] = fsum[(int64_t)g * kFitSums + j];
    if (sums) {
#pragma unroll
      for (int j = 0; j < kFitSums; ++j) sums[(int64_t)g * kFitSums + j] = a[j];
    }
    fit_solve(a, ss + 2 * (int64_t)g);
    return;
  }
  __shared__ double tot[kFitSums];
  frame_order_total<kFitSums>(fsum, F, tot);
  if (sums && threadIdx.x < kFitSums) sums[threadIdx.x] = tot[threadIdx.x];
  if (threadIdx.x == 0) {
    double a[kFitSums];
#pragma unroll
    for (int j = 0; j < kFitSums; ++j) a[j] = tot[j];
    fit_solve(a, ss);
  }
}

// total[j] = frame_sums[0][j] + frame_sums[1][j] + ... in frame order.
__global__ __launch_bounds__(64) void metric_total_kernel(const double* __restrict__ frame_sums, int F,
                                                          double* __restrict__ total) {
  __shared__ double tot[kMetricSums];
  frame_order_total<kMetricSums>(frame_sums, F, tot);
  if (threadIdx.x < kMetricSums) total[threadIdx.x] = tot[threadIdx.x];
}

}  // namespace

extern "C" int64_t vda_depth_eval_workspace(int32_t F, int64_t S) {
  if (F < 1 || S < 1) return 0;
  const int64_t doubles = (int64_t)F * blocks_per_frame(S) * kPartStride + (int64_t)F * kFitSums;
  return (doubles * (int64_t)sizeof(double) + 255) / 256 * 256;
}

extern "C" int vda_depth_eval_fit(const float* pred, const float* gt, const uint8_t* valid, int32_t F, int64_t S,
                                  int32_t per_frame, double* sums, float* ss, void* ws, int64_t ws_bytes,
                                  void* stream) {
  VDA_CHECK_ARG(pred && gt && ss && ws, "null pointer");
  VDA_CHECK_ARG(F >= 1 && S >= 1, "depth_eval_fit needs F >= 1 and S >= 1");
  VDA_CHECK_ARG(F <= kMaxFrames, "depth_eval_fit takes F <= 65535 frames per call");
  VDA_CHECK_ARG(((uintptr_t)pred & 3) == 0 && ((uintptr_t)gt & 3) == 0 && ((uintptr_t)ss & 3) == 0 &&
                    ((uintptr_t)sums & 7) == 0 && ((uintptr_t)ws & 7) == 0,
                "pred / gt / ss must be 4-byte aligned, sums and the workspace 8-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_depth_eval_workspace(F, S), "workspace smaller than vda_depth_eval_workspace(F, S)");
  const int B = blocks_per_frame(S);
  double* part = (double*)ws;
  double* fsum = part + (int64_t)F * B * kPartStride;
  const dim3 grid(B, F), block(kStreamBlock);
  if (valid)
    hipLaunchKernelGGL((eval_partial_kernel<false, true>), grid, block, 0, (hipStream_t)stream, pred, gt, valid, S,
                       (const float*)nullptr, 0, 0.f, (float*)nullptr, part);
  else
    hipLaunchKernelGGL((eval_partial_kernel<false, false>), grid, block, 0, (hipStream_t)stream, pred, gt, valid, S,
                       (const float*)nullptr, 0, 0.f, (float*)nullptr, part);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_reduce_kernel<kFitSums>, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double*)part, B,
                     fsum);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(fit_solve_kernel, dim3(per_frame ? (F + 63) / 64 : 1), dim3(64), 0, (hipStream_t)stream,
                     (const double*)fsum, F, per_frame ? 1 : 0, sums, ss);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_depth_eval_metrics(const float* pred, const float* gt, const uint8_t* valid, int32_t F, int64_t S,
                                      const float* ss, int32_t ss_per_frame, float max_depth, float* aligned,
                                      double* frame_sums, double* total, void* ws, int64_t ws_bytes, void* stream) {
  VDA_CHECK_ARG(pred && gt && ss && frame_sums && ws, "null pointer");
  VDA_CHECK_ARG(F >= 1 && S >= 1, "depth_eval_metrics needs F >= 1 and S >= 1");
  VDA_CHECK_ARG(F <= kMaxFrames, "depth_eval_metrics takes F <= 65535 frames per call");
  VDA_CHECK_ARG(max_depth > 0.f, "depth_eval_metrics needs max_depth > 0");
  VDA_CHECK_ARG(((uintptr_t)pred & 3) == 0 && ((uintptr_t)gt & 3) == 0 && ((uintptr_t)ss & 3) == 0 &&
                    ((uintptr_t)aligned & 3) == 0 && ((uintptr_t)frame_sums & 7) == 0 && ((uintptr_t)total & 7) == 0 &&
                    ((uintptr_t)ws & 7) == 0,
                "pred / gt / ss / aligned must be 4-byte aligned, frame_sums, total and the workspace 8-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_depth_eval_workspace(F, S), "workspace smaller than vda_depth_eval_workspace(F, S)");
  const int B = blocks_per_frame(S);
  double* part = (double*)ws;
  const dim3 grid(B, F), block(kStreamBlock);
  if (valid)
    hipLaunchKernelGGL((eval_partial_kernel<true, true>), grid, block, 0, (hipStream_t)stream, pred, gt, valid, S, ss,
                       ss_per_frame ? 1 : 0, max_depth, aligned, part);
  else
    hipLaunchKernelGGL((eval_partial_kernel<true, false>), grid, block, 0, (hipStream_t)stream, pred, gt, valid, S,
                       ss, ss_per_frame ? 1 : 0, max_depth, aligned, part);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_reduce_kernel<kMetricSums>, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double*)part, B,
                     frame_sums);
  VDA_LAUNCH_CHECK();
  if (total) {
    hipLaunchKernelGGL(metric_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)frame_sums, F, total);
    VDA_LAUNCH_CHECK();
  }
  return 0;
}
