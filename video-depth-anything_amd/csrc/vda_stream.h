// The streaming pass: the skeleton shared by the HBM-bound, one-pass kernels over a flat run of n fp32
// elements (vda_align.hip, vda_eval.hip, vda_vis.hip, vda_compare.hip).  What a kernel does with an element
// is its own; how the run is cut up, walked and reduced is defined here and nowhere else.
//
// The split.  A run is head + 4 * nvec + tail elements: the head (0..3) ends at the first boundary the
// body's vector access needs, the body is nvec groups of 4, the tail (0..3) is what is left.  Two rules
// say where the boundary is: the 16-byte load of the fp32 source (stream_split_f32), or the dword store
// of a byte destination (stream_split_u8).  Other operands of the body share that head and are accessed
// through the element-aligned vector types of vda_common.h.
// The walk.  stream_walk takes the groups grid-stride over gridDim.x blocks of kStreamBlock threads,
// one group per thread and iteration; block 0 also takes the edges, one element per thread: threads
// 0..head-1 the head, threads 8..8+tail-1 the tail.  Every element is visited exactly once.
// The reduction.  Deterministic, no atomics: per thread -> wave butterfly -> the block's waves added in
// wave order (block_store_partial) -> per-block partials in the caller's workspace -> one wave adds the
// partials in index order (wave_add_partials).  The number of blocks (stream_grid) is therefore part of
// the summation order and of the workspace size.  Minima and maxima (block_store_range) take the same two
// stages; they are order-independent, so their result is exact.
#pragma once
#include "vda_common.h"

constexpr int kStreamBlock = 256;
constexpr int kStreamWaves = kStreamBlock / 64;
constexpr int64_t kStreamGroup = (int64_t)kStreamBlock * 4;  // elements per block and iteration

// Blocks for n elements at `span` elements per block: ceil(n / span), at least 1, at most cap.
inline int stream_grid(int64_t n, int64_t span, int64_t cap) {
  const int64_t want = (n + span - 1) / span;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

struct StreamSplit {
  int64_t head;  // elements before the first boundary, at most n
  int64_t nvec;  // groups of 4 after it
};
__device__ __forceinline__ StreamSplit stream_split(int64_t head, int64_t n) {
  if (head > n) head = n;
  return {head, (n - head) / 4};
}
// The boundary is 16 bytes on the fp32 source (4-byte aligned).
__device__ __forceinline__ StreamSplit stream_split_f32(const float* src, int64_t n) {
  return stream_split((int64_t)((16 - ((uintptr_t)src & 15)) & 15) / 4, n);
}
// The boundary is 4 bytes on a byte destination where element e lies at dst + bpe * e, bpe = 1 or 3.
// One byte per element: the head is the bytes up to the boundary.  Three (interleaved RGB): 3 h = -h
// mod 4, so the head is (dst & 3) elements.
__device__ __forceinline__ StreamSplit stream_split_u8(const uint8_t* dst, int bpe, int64_t n) {
  const int64_t a = (int64_t)((uintptr_t)dst & 3);
  return stream_split(bpe == 3 ? a : (4 - a) & 3, n);
}

// body(o): the group of 4 elements o .. o + 3, o = head + 4 i.  edge(e): the single element e.
template <class Body, class Edge>
__device__ __forceinline__ void stream_walk(int64_t n, int64_t head, int64_t nvec, Body&& body, Edge&& edge) {
  const int64_t stride = (int64_t)gridDim.x * kStreamBlock;
  for (int64_t i = (int64_t)blockIdx.x * kStreamBlock + threadIdx.x; i < nvec; i += stride) body(head + 4 * i);
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + 4 * nvec;
    const int tail = (int)(n - tail0);  // 0..3
    int64_t e = -1;
    if ((int64_t)threadIdx.x < head) e = threadIdx.x;
    else if ((int)threadIdx.x >= 8 && (int)threadIdx.x - 8 < tail) e = tail0 + (threadIdx.x - 8);
    if (e >= 0) edge(e);
  }
}

// The block's K sums to part[0..K-1]: wave butterfly, then the waves added 0, 1, 2, 3.
template <int K>
__device__ __forceinline__ void block_store_partial(const double (&s)[K], double* __restrict__ part) {
  __shared__ double red[kStreamWaves][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double w = wave_sum_f64(s[j]);
    if (lane == 0) red[wave][j] = w;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double a = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kStreamWaves; ++w) a += red[w][threadIdx.x];
    part[threadIdx.x] = a;
  }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// The block's (min, max) to out[0], out[1]: waves through LDS, thread 0 stores.
__device__ __forceinline__ void block_store_range(float mn, float mx, float* __restrict__ out) {
  __shared__ float red[kStreamWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (lane == 0) {
    red[wave][0] = mn;
    red[wave][1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kStreamWaves; ++w) {
      mn = fminf(mn, red[w][0]);
      mx = fmaxf(mx, red[w][1]);
    }
    out[0] = mn;
    out[1] = mx;
  }
}

// One block: the (min, max) of the nparts block partials at part [nparts, 2] to range[0], range[1].
__device__ __forceinline__ void block_reduce_ranges(const float* __restrict__ part, int nparts,
                                                    float* __restrict__ range) {
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int b = threadIdx.x; b < nparts; b += kStreamBlock) {
    mn = fminf(mn, part[2 * b]);
    mx = fmaxf(mx, part[2 * b + 1]);
  }
  block_store_range(mn, mx, range);
}

// One wave: lane l adds partials l, l + 64, ... (partial b at part[b * stride ..]) in index order, a
// butterfly adds the lanes; every lane gets sum j as done(j, sum), j = 0..K-1 in turn.
template <int K, class Done>
__device__ __forceinline__ void wave_add_partials(const double* __restrict__ part, int nparts, int stride,
                                                  Done&& done) {
  double a[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = 0.;
  for (int b = threadIdx.x; b < nparts; b += 64) {
#pragma unroll
    for (int j = 0; j < K; ++j) a[j] += part[(int64_t)b * stride + j];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) done(j, wave_sum_f64(a[j]));
}

// The 2x2 normal equations [a00 a01; a01 a11] x = [b0; b1] of a = {a00, a01, a11, b0, b1} in fp64: the
// plain closed form, no contraction.  False, and x untouched, when the system is singular.
__device__ __forceinline__ bool solve_2x2(const double (&a)[5], double& x0, double& x1) {
#pragma clang fp contract(off)
  const double a00 = a[0], a01 = a[1], a11 = a[2], b0 = a[3], b1 = a[4];
  const double det = a00 * a11 - a01 * a01;
  if (det != 0.) {
    x0 = (a11 * b0 - a01 * b1) / det;
    x1 = (-a01 * b0 + a00 * b1) / det;
  }
  return det != 0.;
}
