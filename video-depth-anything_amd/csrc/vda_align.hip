// Scale/shift alignment of depth windows on the device: the least-squares statistics and the
// resize + affine + clip + blend pass around them.
//
// scale_shift: compute_scale_and_shift (utils/util.py:40-62) as video_depth.py:393-395 (long video)
// and :312-314 (streaming) call it: five masked sums over pred / target and the 2x2 solve.  The
// reference sums in fp32 in numpy's pairwise order; here every sum is fp64 in the fixed order of the
// streaming pass (vda_stream.h: 16-byte loads on pred, element-aligned ones on target / mask), and one
// wave adds the partials and solves, so the result is the same bits on every run and no atomics are
// involved.  HBM-bound: 8 B (9 B with a mask) per element.
//
// depth_align: video_depth.py:371 / :299 (resize) + :400-413 / :315 (affine, clip) + get_interpolate_frames
// (utils/util.py:65-73, blend) in one pass, one thread per output pixel: the resized, unaligned
// window is never written to HBM.  4 B read (through L1/L2) + 4 B written per element, + 4 B with a blend.
#include "vda_stream.h"
#include "../../include/vda.h"

namespace {

struct Sums {
  double v[5];  // a_00 = S m p^2, a_01 = S m p, a_11 = S m, b_0 = S m p t, b_1 = S m t
};

__device__ __forceinline__ void accumulate(Sums& s, float p, float t, float m) {
  const double dp = (double)p, dt = (double)t, dm = (double)m;
  const double mp = dm * dp;  // exact: a product of two fp32 values
  s.v[0] = fma(mp, dp, s.v[0]);
  s.v[1] += mp;
  s.v[2] += dm;
  s.v[3] = fma(mp, dt, s.v[3]);
  s.v[4] = fma(dm, dt, s.v[4]);
}

// One 16-byte group per thread and iteration, at most 4 blocks per CU.
int scale_shift_grid(int64_t n) { return stream_grid(n, kStreamGroup, 4 * (int64_t)vda_cu_count()); }

// Block b leaves its five sums in part[b * 5 .. b * 5 + 4]; the split is pred's.
template <bool MASK>
__global__ __launch_bounds__(kStreamBlock) void scale_shift_partial_kernel(const float* __restrict__ pred,
                                                                           const float* __restrict__ target,
                                                                           const uint8_t* __restrict__ mask, int64_t n,
                                                                           double* __restrict__ part) {
  Sums s = {{0., 0., 0., 0., 0.}};
  const StreamSplit sp = stream_split_f32(pred, n);
  stream_walk(
      n, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4 p = *reinterpret_cast<const f4*>(pred + o);
        const f4a4 t = *reinterpret_cast<const f4a4*>(target + o);
        float m[4] = {1.f, 1.f, 1.f, 1.f};
        if (MASK) {
          const u8x4a1 mv = *reinterpret_cast<const u8x4a1*>(mask + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) m[j] = (float)mv[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) accumulate(s, p[j], t[j], m[j]);
      },
      [&](int64_t e) { accumulate(s, pred[e], target[e], MASK ? (float)mask[e] : 1.f); });
  block_store_partial<5>(s.v, part + (int64_t)blockIdx.x * 5);
}

// One wave adds the partials, lane 0 solves the 2x2 system (singular: the identity) and rounds once on
// the store.
__global__ __launch_bounds__(64) void scale_shift_solve_kernel(const double* __restrict__ part, int nparts,
                                                               double* __restrict__ sums, float* __restrict__ ss) {
  double a[5];
  wave_add_partials<5>(part, nparts, 5, [&](int j, double v) { a[j] = v; });
  if (threadIdx.x == 0) {
    double x0 = 1., x1 = 0.;
    solve_2x2(a, x0, x1);
    if (sums) {
#pragma unroll
      for (int j = 0; j < 5; ++j) sums[j] = a[j];
    }
    ss[0] = (float)x0;
    ss[1] = (float)x1;
  }
}

// numpy's `d * scale + shift` and `pre * (1 - w) + post * w` on float32 arrays round every multiply
// and every add on its own; a contracted fma would not match them.
__device__ __forceinline__ float affine_rn(float r, float scale, float shift) {
#pragma clang fp contract(off)
  const float m = r * scale;
  return m + shift;
}
__device__ __forceinline__ float blend_rn(float pre, float w_pre, float post, float w_post) {
#pragma clang fp contract(off)
  const float a = pre * w_pre;
  const float b = post * w_post;
  return a + b;
}

constexpr int kMaxAlignFrames = 32;
struct BlendArgs {
  float w_pre[kMaxAlignFrames];
  float w_post[kMaxAlignFrames];
};

// pre and out may be the same buffer: every thread reads its own pre element before it stores.
__global__ __launch_bounds__(256) void depth_align_kernel(const float* __restrict__ src, const float* __restrict__ ss,
                                                          const float* pre, float* out, int H, int W, int ho, int wo,
                                                          int clip, BlendArgs ba) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  const int oy = blockIdx.y;
  const int n = blockIdx.z;
  if (ox >= wo) return;
  float v = depth_bilinear_ac(src + (size_t)n * H * W, H, W, ho, wo, oy, ox);
  if (ss) v = affine_rn(v, ss[0], ss[1]);
  if (clip) v = v < 0.f ? 0.f : v;
  const size_t o = ((size_t)n * ho + oy) * wo + ox;
  if (pre) v = blend_rn(pre[o], ba.w_pre[n], v, ba.w_post[n]);
  out[o] = v;
}

}  // namespace

extern "C" int64_t vda_scale_shift_workspace(int64_t n) {
  if (n < 1) return 0;
  return ((int64_t)scale_shift_grid(n) * 5 * (int64_t)sizeof(double) + 255) / 256 * 256;
}

extern "C" int vda_scale_shift(const float* pred, const float* target, const uint8_t* mask, int64_t n, double* sums,
                               float* ss, void* ws, int64_t ws_bytes, void* stream) {
  VDA_CHECK_ARG(pred && target && ss && ws, "null pointer");
  VDA_CHECK_ARG(n >= 1, "scale_shift needs n >= 1");
  VDA_CHECK_ARG(((uintptr_t)pred & 3) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)ws & 7) == 0 &&
                    ((uintptr_t)sums & 7) == 0 && ((uintptr_t)ss & 3) == 0,
                "pred / target / ss must be 4-byte aligned, sums and the workspace 8-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_scale_shift_workspace(n), "workspace smaller than vda_scale_shift_workspace(n)");
  const int grid = scale_shift_grid(n);
  double* part = (double*)ws;
  if (mask)
    hipLaunchKernelGGL(scale_shift_partial_kernel<true>, dim3(grid), dim3(kStreamBlock), 0, (hipStream_t)stream, pred,
                       target, mask, n, part);
  else
    hipLaunchKernelGGL(scale_shift_partial_kernel<false>, dim3(grid), dim3(kStreamBlock), 0, (hipStream_t)stream, pred,
                       target, mask, n, part);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(scale_shift_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)part, grid, sums,
                     ss);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_depth_align(const float* src, int32_t F, int32_t H, int32_t W, int32_t ho, int32_t wo, const float* ss,
                               int32_t clip, const float* pre, const float* w_pre, const float* w_post, float* out,
                               void* stream) {
  VDA_CHECK_ARG(src && out, "null pointer");
  VDA_CHECK_ARG(F > 0 && H > 0 && W > 0 && ho > 0 && wo > 0, "empty depth geometry");
  VDA_CHECK_ARG(F <= kMaxAlignFrames, "depth_align takes F <= 32 frames per call");
  VDA_CHECK_ARG(ho <= 65535, "output height exceeds the launch grid");
  VDA_CHECK_ARG(!pre || (w_pre && w_post), "a blend (pre) needs the host weight arrays w_pre and w_post");
  BlendArgs ba;
  for (int f = 0; f < kMaxAlignFrames; ++f) {
    ba.w_pre[f] = pre && f < F ? w_pre[f] : 0.f;
    ba.w_post[f] = pre && f < F ? w_post[f] : 0.f;
  }
  hipLaunchKernelGGL(depth_align_kernel, dim3((wo + 255) / 256, ho, F), dim3(256), 0, (hipStream_t)stream, src, ss, pre,
                     out, H, W, ho, wo, clip ? 1 : 0, ba);
  VDA_LAUNCH_CHECK();
  return 0;
}
