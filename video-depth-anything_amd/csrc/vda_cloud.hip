// Point clouds on the device: metric depth [F, H, W] through the pinhole intrinsics and a camera-to-output
// matrix per frame to a dense, ordered list of 3-D points (the reference's project_image_to_pointcloud /
// project_scene_to_3d, datasets/visualisation_utils.py:82-187, which go through Open3D on the host), either
// as [N, 3] fp32 + [N, 3] uint8 or as the body of a binary PLY (12- or 15-byte records at any byte address).
//
// It is an order-preserving stream compaction fused with the unprojection, in two passes over the depth:
// count:  a block owns one contiguous run of kSpan candidates of one frame (never grid-stride: ownership
//         follows candidate order) and counts the ones it keeps; a scan per frame and a scan over the frames
//         turn the counts into each block's output offset (in the caller's workspace, which carries them to
//         the second pass) and into frame_offsets.  Integer sums, no atomics.
// write:  the same blocks recompute the predicate.  In iteration t lane l of wave w owns candidate
//         t * 256 + 64 w + l of the block's run, so inside a wave the rank of a kept lane is the popcount of
//         the 64-bit ballot below it, and the (t, w) groups follow each other in candidate order: their counts
//         go through LDS and every thread adds up the groups before its own.  The block's records are
//         staged in LDS at the byte phase of their destination and leave as one contiguous byte run: bytes
//         up to the first dword boundary, dwords, bytes after the last (the edge rule of vda_depth_colorize).
// Per point every operation is one correctly rounded fp32 operation (IEEE division, no reciprocal, no
// contraction), so the result equals the separate torch fp32 ops bit for bit.  Dropped candidates are selected
// out by compares (NaN, +-Inf, 0 and negative depths fail them), never multiplied out.
// HBM-bound: count reads 4 (+1) B per candidate, write 4 (+1) B per candidate and 3 B per kept point, and
// stores 12 / 15 B per kept point.
#include "vda_common.h"
#include "../../include/vda.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kIters = 4;                    // candidates per thread
constexpr int kSpan = kBlock * kIters;       // candidates per block
constexpr int kGroups = kIters * kWaves;     // (iteration, wave) groups of 64 candidates, in candidate order
constexpr int kMaxFrames = 65535;            // grid.y
constexpr int kMaxRecord = 15;
constexpr int kStageBytes = kSpan * kMaxRecord + 4;  // + the byte phase of the destination (0..3)

struct Grid {
  int32_t hs, ws;   // candidate rows and columns of a frame
  int64_t cand;     // hs * ws
  int64_t blocks;   // per frame
};
Grid cloud_grid(int32_t H, int32_t W, int32_t step) {
  Grid g;
  g.hs = (int32_t)(((int64_t)H + step - 1) / step);
  g.ws = (int32_t)(((int64_t)W + step - 1) / step);
  g.cand = (int64_t)g.hs * g.ws;
  g.blocks = (g.cand + kSpan - 1) / kSpan;
  return g;
}

// What a block knows about its run: frame f, candidates c0 .. c0 + n - 1 of the frame's cand, the first
// one at candidate row r0, column q0.
struct Run {
  int64_t f, c0;
  int32_t n, r0, q0;
};
__device__ __forceinline__ Run block_run(int64_t cand, int32_t ws) {
  Run r;
  r.f = blockIdx.y;
  r.c0 = (int64_t)blockIdx.x * kSpan;
  const int64_t left = cand - r.c0;
  r.n = (int32_t)(left < kSpan ? left : kSpan);
  r.r0 = (int32_t)(r.c0 / ws);
  r.q0 = (int32_t)(r.c0 - (int64_t)r.r0 * ws);
  return r;
}
// Candidate l of the run -> pixel (i, j).  q0 + l < 2^31 + kSpan, so the division is a 32-bit one.
__device__ __forceinline__ void run_pixel(const Run& r, int32_t l, int32_t ws, int32_t step, int32_t& i, int32_t& j) {
  const uint32_t q = (uint32_t)r.q0 + (uint32_t)l;
  const uint32_t dr = q / (uint32_t)ws;
  i = (int32_t)((uint32_t)r.r0 + dr) * step;
  j = (int32_t)(q - dr * (uint32_t)ws) * step;
}

__device__ __forceinline__ bool keep_depth(float d, float trunc) { return d > 0.0f && d < trunc; }

// The depths and the keep flags of this thread's kIters candidates; flag t is bit t of the result.
template <bool MASK>
__device__ __forceinline__ uint32_t load_run(const Run& r, const float* __restrict__ depth,
                                             const uint8_t* __restrict__ valid, int32_t H, int32_t W, int32_t ws,
                                             int32_t step, float trunc, float (&d)[kIters], int64_t (&pix)[kIters]) {
  const int64_t frame = r.f * (int64_t)H * W;
  uint8_t m[kIters];
#pragma unroll
  for (int t = 0; t < kIters; ++t) {
    const int32_t l = t * kBlock + (int32_t)threadIdx.x;
    d[t] = 0.f;
    m[t] = 0;
    pix[t] = 0;
    if (l < r.n) {
      if (step == 1) {  // the candidates are the pixels
        pix[t] = frame + r.c0 + l;
      } else {
        int32_t i, j;
        run_pixel(r, l, ws, step, i, j);
        pix[t] = frame + (int64_t)i * W + j;
      }
      d[t] = depth[pix[t]];
      m[t] = MASK ? valid[pix[t]] : 1;
    }
  }
  uint32_t keep = 0;
#pragma unroll
  for (int t = 0; t < kIters; ++t) keep |= (m[t] != 0 && keep_depth(d[t], trunc)) ? 1u << t : 0u;
  return keep;
}

// off[f * gridDim.x + b] = kept candidates of block b of frame f.
template <bool MASK>
__global__ __launch_bounds__(kBlock) void cloud_count_kernel(const float* __restrict__ depth,
                                                             const uint8_t* __restrict__ valid, int32_t H, int32_t W,
                                                             int32_t ws, int64_t cand, int32_t step, float trunc,
                                                             int64_t* __restrict__ off) {
  __shared__ int32_t wc[kWaves];
  const Run r = block_run(cand, ws);
  float d[kIters];
  int64_t pix[kIters];
  const uint32_t keep = load_run<MASK>(r, depth, valid, H, W, ws, step, trunc, d, pix);
  int32_t n = 0;
#pragma unroll
  for (int t = 0; t < kIters; ++t) n += __popcll(__ballot((keep >> t) & 1));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wc[w];
    off[r.f * gridDim.x + blockIdx.x] = s;
  }
}

// One block: a[0..n-1] becomes its exclusive prefix in place; returns the total to every thread.
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t* __restrict__ a, int64_t n) {
  __shared__ int64_t wt[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += kBlock) {
    const int64_t k = base + threadIdx.x;
    const int64_t v = k < n ? a[k] : 0;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wt[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? wt[w] : 0;
      all += wt[w];
    }
    if (k < n) a[k] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  return carry;
}

// Frame f = blockIdx.x: its blocks' counts -> offsets inside the frame; ftot[f] = the frame's count.
__global__ __launch_bounds__(kBlock) void cloud_frame_scan_kernel(int64_t* __restrict__ off, int64_t blocks,
                                                                  int64_t* __restrict__ ftot) {
  const int64_t f = blockIdx.x;
  const int64_t total = block_exclusive_scan(off + f * blocks, blocks);
  if (threadIdx.x == 0) ftot[f] = total;
}

// One block: the frames' counts -> the frames' offsets, in ftot for the write pass and in frame_offsets [F + 1].
__global__ __launch_bounds__(kBlock) void cloud_frames_scan_kernel(int64_t* __restrict__ ftot, int32_t F,
                                                                   int64_t* __restrict__ frame_offsets) {
  const int64_t total = block_exclusive_scan(ftot, F);
  __syncthreads();  // this block's own stores to ftot, read back by other threads
  for (int32_t f = threadIdx.x; f < F; f += kBlock) frame_offsets[f] = ftot[f];
  if (threadIdx.x == 0) frame_offsets[F] = total;
}

// A float into the LDS staging area (dword-aligned itself) at any byte offset o.
__device__ __forceinline__ void stage_f32(uint8_t* stage, int32_t o, float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  uint8_t* p = stage + o;
  if ((o & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = u;
  } else {
    p[0] = (uint8_t)u;
    p[1] = (uint8_t)(u >> 8);
    p[2] = (uint8_t)(u >> 16);
    p[3] = (uint8_t)(u >> 24);
  }
}

// The n bytes staged at lds[a .. a + n - 1], a = dst & 3, to dst .. dst + n - 1: LDS dword q and global dword q
// (from dst - a) hold the same bytes, so the run leaves as bytes up to the first boundary, dwords, and bytes.
__device__ __forceinline__ void flush_run(const uint8_t* lds, uint8_t* __restrict__ dst, int32_t a, int64_t n) {
  uint8_t* g0 = dst - a;
  const int64_t end = a + n;
  const int64_t q0 = a ? 1 : 0, q1 = end >> 2;
  const int64_t head_end = 4 * q0 < end ? 4 * q0 : end;
  const int64_t tail0 = 4 * q1 > head_end ? 4 * q1 : head_end;
  const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lds);
  for (int64_t q = q0 + threadIdx.x; q < q1; q += kBlock) *reinterpret_cast<uint32_t*>(g0 + 4 * q) = l32[q];
  const int64_t h = a + (int64_t)threadIdx.x;
  if (h < head_end) g0[h] = lds[h];
  const int64_t e = tail0 + ((int64_t)threadIdx.x - 8);
  if ((int)threadIdx.x >= 8 && e < end) g0[e] = lds[e];
}

// PACKED: out = records of 12 (+ 3 with RGB) bytes at any address.  Otherwise out = float [cap, 3] and
// out_rgb = uint8 [cap, 3].  off / fbase: what the count pass left in the workspace.
template <bool MASK, bool RGB, bool XFORM, bool PACKED>
__global__ __launch_bounds__(kBlock) void cloud_write_kernel(const float* __restrict__ depth,
                                                             const uint8_t* __restrict__ valid,
                                                             const uint8_t* __restrict__ rgb, int32_t H, int32_t W,
                                                             int32_t ws, int64_t cand, int32_t step, float trunc,
                                                             const float* __restrict__ Kf, const float* __restrict__ Mf,
                                                             uint8_t* __restrict__ out, uint8_t* __restrict__ out_rgb,
                                                             int64_t cap, const int64_t* __restrict__ off,
                                                             const int64_t* __restrict__ fbase) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  __shared__ int32_t gc[kGroups];
  const Run r = block_run(cand, ws);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float d[kIters];
  int64_t pix[kIters];
  const uint32_t keep = load_run<MASK>(r, depth, valid, H, W, ws, step, trunc, d, pix);
  int32_t rank[kIters];
#pragma unroll
  for (int t = 0; t < kIters; ++t) {
    const uint64_t b = __ballot((keep >> t) & 1);
    rank[t] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) gc[t * kWaves + wave] = __popcll(b);
  }
  __syncthreads();
  // groups in candidate order: g = t * kWaves + wave.  base[t] = the kept candidates of the groups before g.
  int32_t base[kIters];
  int32_t run = 0;
#pragma unroll
  for (int t = 0; t < kIters; ++t) {
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int32_t c = gc[t * kWaves + w];
      before += w < wave ? c : 0;
      all += c;
    }
    base[t] = run + before;
    run += all;
  }
  const int64_t first = fbase[r.f] + off[r.f * gridDim.x + blockIdx.x];  // this block's first point
  int64_t room = cap - first;
  room = room < 0 ? 0 : room;
  const int32_t nrec = (int32_t)(room < run ? room : run);  // records this block may store
  if (nrec == 0) return;

  constexpr int kRec = PACKED ? (RGB ? 15 : 12) : 12;
  uint8_t* dst = out + first * kRec;
  const int32_t a = PACKED ? (int32_t)((uintptr_t)dst & 3) : 0;
  // SPLIT with RGB: the colours are a second run behind the points' kSpan * 12 bytes (+ its own phase)
  uint8_t* dst_c = (!PACKED && RGB) ? out_rgb + first * 3 : nullptr;
  const int32_t ac = (!PACKED && RGB) ? (int32_t)((uintptr_t)dst_c & 3) : 0;
  uint8_t* stage_c = stage + kSpan * 12;

  const float fx = Kf[4 * r.f + 0], fy = Kf[4 * r.f + 1], cx = Kf[4 * r.f + 2], cy = Kf[4 * r.f + 3];
  float m[12];
  if (XFORM) {
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = Mf[12 * r.f + k];
  }
#pragma unroll
  for (int t = 0; t < kIters; ++t) {
    const int32_t k = base[t] + rank[t];
    if (((keep >> t) & 1) && k < nrec) {
      int32_t i, j;
      run_pixel(r, t * kBlock + (int32_t)threadIdx.x, ws, step, i, j);
      const float z = d[t];
      const float x = (((float)j - cx) * z) / fx;
      const float y = (((float)i - cy) * z) / fy;
      float p[3] = {x, y, z};
      if (XFORM) {
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = ((m[4 * q] * x + m[4 * q + 1] * y) + m[4 * q + 2] * z) + m[4 * q + 3];
      }
      const int32_t o = a + k * kRec;
      stage_f32(stage, o, p[0]);
      stage_f32(stage, o + 4, p[1]);
      stage_f32(stage, o + 8, p[2]);
      if (RGB) {
        const uint8_t* c = rgb + 3 * pix[t];
        uint8_t* sc = PACKED ? stage + o + 12 : stage_c + ac + k * 3;
        sc[0] = c[0];
        sc[1] = c[1];
        sc[2] = c[2];
      }
    }
  }
  __syncthreads();
  flush_run(stage, dst, a, (int64_t)nrec * kRec);
  if (!PACKED && RGB) flush_run(stage_c, dst_c, ac, (int64_t)nrec * 3);
}

template <bool MASK, bool RGB, bool XFORM>
void launch_write(int32_t layout, dim3 grid, hipStream_t st, const float* depth, const uint8_t* valid,
                  const uint8_t* rgb, int32_t H, int32_t W, const Grid& g, int32_t step, float trunc, const float* K,
                  const float* M, uint8_t* out, uint8_t* out_rgb, int64_t cap, const int64_t* off,
                  const int64_t* fbase) {
  if (layout == VDA_CLOUD_PACKED)
    hipLaunchKernelGGL((cloud_write_kernel<MASK, RGB, XFORM, true>), grid, dim3(kBlock), 0, st, depth, valid, rgb, H, W,
                       g.ws, g.cand, step, trunc, K, M, out, out_rgb, cap, off, fbase);
  else
    hipLaunchKernelGGL((cloud_write_kernel<MASK, RGB, XFORM, false>), grid, dim3(kBlock), 0, st, depth, valid, rgb, H,
                       W, g.ws, g.cand, step, trunc, K, M, out, out_rgb, cap, off, fbase);
}

// The checks count and write share.  Grids: x up to 2^31 - 1 blocks, and HIP counts threads in 32 bits.
int check_shape(int32_t F, int32_t H, int32_t W, int32_t step) {
  VDA_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && step >= 1, "cloud needs F >= 1, H >= 1, W >= 1 and step >= 1");
  VDA_CHECK_ARG(F <= kMaxFrames, "cloud takes F <= 65535 frames per call");
  VDA_CHECK_ARG(cloud_grid(H, W, step).cand <= INT32_MAX, "cloud takes at most 2^31 - 1 candidates per frame");
  return 0;
}

}  // namespace

extern "C" int64_t vda_cloud_span(void) { return kSpan; }

extern "C" int64_t vda_cloud_workspace(int32_t F, int32_t H, int32_t W, int32_t step) {
  if (F < 1 || H < 1 || W < 1 || step < 1) return 0;
  return ((int64_t)F * cloud_grid(H, W, step).blocks + F) * (int64_t)sizeof(int64_t);
}

extern "C" int vda_cloud_count(const float* depth, const uint8_t* valid, int32_t F, int32_t H, int32_t W,
                               int32_t step, float trunc, int64_t* frame_offsets, void* ws, int64_t ws_bytes,
                               void* stream) {
  VDA_CHECK_ARG(depth && frame_offsets && ws, "null pointer");
  if (int rc = check_shape(F, H, W, step)) return rc;
  VDA_CHECK_ARG(((uintptr_t)depth & 3) == 0 && ((uintptr_t)frame_offsets & 7) == 0 && ((uintptr_t)ws & 7) == 0,
                "depth must be 4-byte aligned, frame_offsets and the workspace 8-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_cloud_workspace(F, H, W, step), "workspace smaller than vda_cloud_workspace(F, H, W, step)");
  const Grid g = cloud_grid(H, W, step);
  int64_t* off = (int64_t*)ws;
  int64_t* ftot = off + (int64_t)F * g.blocks;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((uint32_t)g.blocks, F), block(kBlock);
  if (valid)
    hipLaunchKernelGGL(cloud_count_kernel<true>, grid, block, 0, st, depth, valid, H, W, g.ws, g.cand, step, trunc, off);
  else
    hipLaunchKernelGGL(cloud_count_kernel<false>, grid, block, 0, st, depth, valid, H, W, g.ws, g.cand, step, trunc, off);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_frame_scan_kernel, dim3(F), block, 0, st, off, g.blocks, ftot);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_frames_scan_kernel, dim3(1), block, 0, st, ftot, F, frame_offsets);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_cloud_write(const float* depth, const uint8_t* valid, const uint8_t* rgb, int32_t F, int32_t H,
                               int32_t W, int32_t step, float trunc, const float* K, const float* M, int32_t layout,
                               void* out, uint8_t* out_rgb, int64_t cap, const void* ws, int64_t ws_bytes,
                               void* stream) {
  VDA_CHECK_ARG(depth && K && ws, "null pointer");
  if (int rc = check_shape(F, H, W, step)) return rc;
  VDA_CHECK_ARG(layout == VDA_CLOUD_SPLIT || layout == VDA_CLOUD_PACKED, "unknown layout (VDA_CLOUD_SPLIT or VDA_CLOUD_PACKED)");
  VDA_CHECK_ARG(cap >= 0, "cloud_write needs cap >= 0");
  VDA_CHECK_ARG(out || cap == 0, "cloud_write needs out unless cap is 0");
  VDA_CHECK_ARG(layout != VDA_CLOUD_SPLIT || !rgb || out_rgb || cap == 0, "VDA_CLOUD_SPLIT with rgb needs out_rgb");
  VDA_CHECK_ARG(((uintptr_t)depth & 3) == 0 && ((uintptr_t)K & 3) == 0 && ((uintptr_t)M & 3) == 0 &&
                    ((uintptr_t)ws & 7) == 0,
                "depth, K and M must be 4-byte aligned, the workspace 8-byte aligned");
  VDA_CHECK_ARG(layout != VDA_CLOUD_SPLIT || ((uintptr_t)out & 3) == 0, "VDA_CLOUD_SPLIT needs a 4-byte aligned out");
  VDA_CHECK_ARG(ws_bytes >= vda_cloud_workspace(F, H, W, step), "workspace smaller than vda_cloud_workspace(F, H, W, step)");
  if (cap == 0) return 0;  // nothing may be stored
  const Grid g = cloud_grid(H, W, step);
  const int64_t* off = (const int64_t*)ws;
  const int64_t* fbase = off + (int64_t)F * g.blocks;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((uint32_t)g.blocks, F);
  const int sel = (valid ? 4 : 0) | (rgb ? 2 : 0) | (M ? 1 : 0);
#define VDA_CLOUD_CASE(S, MASK, RGB, XFORM)                                                                        \
  case S:                                                                                                          \
    launch_write<MASK, RGB, XFORM>(layout, grid, st, depth, valid, rgb, H, W, g, step, trunc, K, M, (uint8_t*)out, \
                                   out_rgb, cap, off, fbase);                                                      \
    break;
  switch (sel) {
    VDA_CLOUD_CASE(0, false, false, false)
    VDA_CLOUD_CASE(1, false, false, true)
    VDA_CLOUD_CASE(2, false, true, false)
    VDA_CLOUD_CASE(3, false, true, true)
    VDA_CLOUD_CASE(4, true, false, false)
    VDA_CLOUD_CASE(5, true, false, true)
    VDA_CLOUD_CASE(6, true, true, false)
    default:
      VDA_CLOUD_CASE(7, true, true, true)
  }
#undef VDA_CLOUD_CASE
  VDA_LAUNCH_CHECK();
  return 0;
}
