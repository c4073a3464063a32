// Depth visualisation on the device: the clip-wide min / max and the colour lookup of the reference's
// save_video (utils/dc_utils.py:74-85), from fp32 depth straight to the bytes that go into the file.
//
// range:    depths.min(), depths.max() (dc_utils.py:76) as a streaming pass (vda_stream.h) with 16-byte
//           loads on depth, a min / max block reduction into per-block partials in the caller's
//           workspace, and one block that reduces the partials.  min / max are order-independent, so the
//           result is exact; NaNs are skipped (fminf / fmaxf).  HBM-bound: 4 B per element read.
// colorize: i = uint8((d - min) / (max - min) * 255) (dc_utils.py:79), every operation one correctly
//           rounded fp32 operation as numpy float32 computes it (IEEE division, no rcp, no contraction),
//           then out = lut[i] in one of four layouts.  The host path makes about eight full-size passes,
//           one of them a float64 [F, H, W, 3] gather; here it is one pass: 4 B read, 1 to 3 B written
//           per pixel.  The table is 256 packed dwords in LDS, staged once per block; the gather's bank
//           conflicts depend on the data (neighbouring pixels of a depth map mostly share an index, which
//           broadcasts, or hit neighbouring entries, which lie on different banks).
// Stores are dwords: frames and planes start at f * H * W and c * H * W bytes, which are not multiples
// of 4 in general, so every plane is a streaming pass of its own (vda_stream.h, split by the dword rule
// on the destination): head, body (groups of 4 pixels, one dword per plane, three dwords for interleaved
// RGB) and tail; the depth loads of the body are element-aligned 16-byte loads.  Planes whose heads differ
// (planar 4:4:4 with H * W % 4 != 0) are written in one pass per plane.  4:2:0: a thread owns a strip of
// four 2x2 blocks (8 x 2 pixels): it looks every pixel up once, stores the luma of both rows and the two
// averaged chroma dwords; a strip whose row address is not dword-aligned, or that is cut by the right
// edge, goes out in the widest aligned stores its address allows (bytes and 16-bit words around dwords;
// none of that at W % 8 == 0 with a dword-aligned output).
#include "vda_stream.h"
#include "../../include/vda.h"

namespace {

constexpr int kMaxFrames = 65535;  // grid.y
// range: a block takes 4 16-byte groups per thread while n is large enough; at most 1,024 blocks
int range_grid(int64_t n) { return stream_grid(n, kStreamGroup * 4, 1024); }
// colorize: 4 groups of 4 pixels per thread and pass while the frame is large enough; at most 512 blocks
// per frame
int color_grid(int64_t S) { return stream_grid(S, kStreamGroup * 4, 512); }

typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));

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

// The split is depth's.  part [gridDim.x, 2].
__global__ __launch_bounds__(kStreamBlock) void range_partial_kernel(const float* __restrict__ depth, int64_t n,
                                                                     float* __restrict__ part) {
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const StreamSplit sp = stream_split_f32(depth, n);
  stream_walk(
      n, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4 d = *reinterpret_cast<const f4*>(depth + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          mn = fminf(mn, d[j]);
          mx = fmaxf(mx, d[j]);
        }
      },
      [&](int64_t e) {
        mn = fminf(mn, depth[e]);
        mx = fmaxf(mx, depth[e]);
      });
  block_store_range(mn, mx, part + 2 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(kStreamBlock) void range_final_kernel(const float* __restrict__ part, int nparts,
                                                                   float* __restrict__ range) {
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int b = threadIdx.x; b < nparts; b += kStreamBlock) {
    mn = fminf(mn, part[2 * b]);
    mx = fmaxf(mx, part[2 * b + 1]);
  }
  block_store_range(mn, mx, range);
}

// dc_utils.py:79 per pixel.  numpy's cast of a NaN, a negative or a too large float to uint8 is undefined;
// here a NaN (0 / 0 for a constant clip) and x < 0 give 0, x > 255 gives 255 (include/vda.h).
__device__ __forceinline__ uint32_t depth_index(float d, float lo, float den) {
#pragma clang fp contract(off)
  const float c = d - lo;
  const float q = c / den;
  const float x = q * 255.0f;
  return x >= 255.f ? 255u : (x > 0.f ? (uint32_t)(int)x : 0u);
}

// The table as 256 dwords r | g << 8 | b << 16 in LDS, one row per thread (lut has no alignment).
__device__ __forceinline__ void stage_table(const uint8_t* __restrict__ lut, uint32_t* tab) {
  const int t = threadIdx.x;
  tab[t] = (uint32_t)lut[3 * t] | ((uint32_t)lut[3 * t + 1] << 8) | ((uint32_t)lut[3 * t + 2] << 16);
  __syncthreads();
}

// NPL planes of one frame that share their alignment: plane c at dst + c * pstride holds, per pixel, the
// index itself (IDX) or byte sel0 + c of its table row.  Head and tail pixels (at most 3 each) are stored
// bytewise by block 0, the body as one dword per plane and group of 4 pixels.
template <int NPL, bool IDX>
__device__ __forceinline__ void planes_pass(const float* __restrict__ df, int64_t S, float lo, float den,
                                            const uint32_t* tab, uint8_t* __restrict__ dst, int64_t pstride,
                                            int sel0) {
  const StreamSplit sp = stream_split_u8(dst, 1, S);
  stream_walk(
      S, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4a4 d = *reinterpret_cast<const f4a4*>(df + o);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t k = depth_index(d[j], lo, den);
          v[j] = IDX ? k : tab[k] >> (8 * sel0);
        }
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
          const uint32_t w = ((v[0] >> (8 * c)) & 0xffu) | (((v[1] >> (8 * c)) & 0xffu) << 8) |
                             (((v[2] >> (8 * c)) & 0xffu) << 16) | (((v[3] >> (8 * c)) & 0xffu) << 24);
          *reinterpret_cast<uint32_t*>(dst + c * pstride + o) = w;
        }
      },
      [&](int64_t e) {
        const uint32_t k = depth_index(df[e], lo, den);
        const uint32_t v = IDX ? k : tab[k] >> (8 * sel0);
#pragma unroll
        for (int c = 0; c < NPL; ++c) dst[c * pstride + e] = (uint8_t)(v >> (8 * c));
      });
}

// Interleaved rows: pixel p of the frame at dst + 3 p.  A group of 4 pixels is 12 bytes = three dwords.
__device__ __forceinline__ void hwc_pass(const float* __restrict__ df, int64_t S, float lo, float den,
                                         const uint32_t* tab, uint8_t* __restrict__ dst) {
  const StreamSplit sp = stream_split_u8(dst, 3, S);
  stream_walk(
      S, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4a4 d = *reinterpret_cast<const f4a4*>(df + o);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tab[depth_index(d[j], lo, den)];  // the top byte is 0
        u32x3a4 w;
        w[0] = v[0] | (v[1] << 24);
        w[1] = (v[1] >> 8) | (v[2] << 16);
        w[2] = (v[2] >> 16) | (v[3] << 8);
        *reinterpret_cast<u32x3a4*>(dst + 3 * o) = w;
      },
      [&](int64_t e) {
        const uint32_t v = tab[depth_index(df[e], lo, den)];
        dst[3 * e] = (uint8_t)v;
        dst[3 * e + 1] = (uint8_t)(v >> 8);
        dst[3 * e + 2] = (uint8_t)(v >> 16);
      });
}

// Frame f = blockIdx.y; the frame's pixels are spread over gridDim.x blocks.
template <int LAYOUT>
__global__ __launch_bounds__(kStreamBlock) void colorize_kernel(const float* __restrict__ depth, int64_t S,
                                                                const float* __restrict__ range,
                                                                const uint8_t* __restrict__ lut,
                                                                uint8_t* __restrict__ out) {
  __shared__ uint32_t tab[256];
  if (LAYOUT != VDA_VIS_INDEX) stage_table(lut, tab);
  const int64_t f = blockIdx.y;
  const float* df = depth + f * S;
  const float lo = range[0];
  const float den = range[1] - lo;
  if (LAYOUT == VDA_VIS_INDEX) {
    planes_pass<1, true>(df, S, lo, den, tab, out + f * S, 0, 0);
  } else if (LAYOUT == VDA_VIS_HWC) {
    hwc_pass(df, S, lo, den, tab, out + 3 * f * S);
  } else {
    uint8_t* of = out + 3 * f * S;
    if ((S & 3) == 0) {  // the three planes share their alignment: one pass
      planes_pass<3, false>(df, S, lo, den, tab, of, S, 0);
    } else {
      for (int c = 0; c < 3; ++c) planes_pass<1, false>(df, S, lo, den, tab, of + c * S, 0, c);
    }
  }
}

// The n <= 8 low bytes of v (low byte first) to p, which has any alignment, in the widest naturally aligned
// stores: a whole dword-aligned strip is two dword stores, one at p % 4 == 2 a 16-bit word, a dword and a
// 16-bit word.  The lanes of a wave mostly share a row, hence p % 4, so the branches are mostly uniform.
__device__ __forceinline__ void store_strip(uint8_t* p, uint64_t v, int n) {
  if (((uintptr_t)p & 1) && n >= 1) {
    *p = (uint8_t)v;
    p += 1, v >>= 8, n -= 1;
  }
  if (((uintptr_t)p & 2) && n >= 2) {
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    p += 2, v >>= 16, n -= 2;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // n >= 4 here only with p dword-aligned
    if (n >= 4) {
      *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
      p += 4, v >>= 32, n -= 4;
    }
  }
  if (n >= 2) {
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    p += 2, v >>= 16, n -= 2;
  }
  if (n >= 1) *p = (uint8_t)v;
}

// 4:2:0: unit u of a frame is the strip of chroma row cy = u / ns, chroma columns 4 g .. 4 g + 3
// (g = u % ns, ns = ceil(cw / 4)): pixels [2 cy, 2 cy + 1] x [8 g, 8 g + 7], rows and columns past the
// edge repeating the last one.
__global__ __launch_bounds__(kStreamBlock) void colorize_420_kernel(const float* __restrict__ depth, int H, int W,
                                                                    const float* __restrict__ range,
                                                                    const uint8_t* __restrict__ lut,
                                                                    uint8_t* __restrict__ out) {
  __shared__ uint32_t tab[256];
  stage_table(lut, tab);
  const int64_t S = (int64_t)H * W;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;
  const int64_t C = (int64_t)ch * cw;
  const int64_t f = blockIdx.y;
  const float* df = depth + f * S;
  uint8_t* yp = out + f * (S + 2 * C);
  uint8_t* up = yp + S;
  uint8_t* vp = up + C;
  const float lo = range[0];
  const float den = range[1] - lo;
  const int64_t ns = (cw + 3) / 4;
  const int64_t units = (int64_t)ch * ns;
  const int64_t stride = (int64_t)gridDim.x * kStreamBlock;
  for (int64_t u = (int64_t)blockIdx.x * kStreamBlock + threadIdx.x; u < units; u += stride) {
    const int cy = (int)(u / ns);
    const int g = (int)(u - (int64_t)cy * ns);
    const int x0 = 8 * g, y0 = 2 * cy;
    const bool two = y0 + 1 < H;
    const int nv = W - x0 < 8 ? W - x0 : 8;        // luma bytes of the strip per row, 1..8
    const int nc = cw - 4 * g < 4 ? cw - 4 * g : 4;  // chroma bytes of the strip per plane, 1..4
    const float* r0 = df + (int64_t)y0 * W + x0;
    const float* r1 = two ? r0 + W : r0;
    uint32_t v[2][8];
    if (nv == 8) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f4a4 a = *reinterpret_cast<const f4a4*>(r0 + 4 * h);
        const f4a4 b = *reinterpret_cast<const f4a4*>(r1 + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[0][4 * h + j] = tab[depth_index(a[j], lo, den)];
          v[1][4 * h + j] = tab[depth_index(b[j], lo, den)];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = j < nv ? j : nv - 1;
        v[0][j] = tab[depth_index(r0[x], lo, den)];
        v[1][j] = tab[depth_index(r1[x], lo, den)];
      }
    }
    uint32_t yw[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        yw[r][h] = (v[r][4 * h] & 0xffu) | ((v[r][4 * h + 1] & 0xffu) << 8) | ((v[r][4 * h + 2] & 0xffu) << 16) |
                   ((v[r][4 * h + 3] & 0xffu) << 24);
    }
    uint8_t* yrow = yp + (int64_t)y0 * W + x0;
    store_strip(yrow, (uint64_t)yw[0][0] | ((uint64_t)yw[0][1] << 32), nv);
    if (two) store_strip(yrow + W, (uint64_t)yw[1][0] | ((uint64_t)yw[1][1] << 32), nv);
    uint32_t uw = 0, vw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t a = v[0][2 * k], b = v[0][2 * k + 1], c = v[1][2 * k], d = v[1][2 * k + 1];
      const uint32_t su = ((a >> 8) & 0xffu) + ((b >> 8) & 0xffu) + ((c >> 8) & 0xffu) + ((d >> 8) & 0xffu) + 2u;
      const uint32_t sv = ((a >> 16) & 0xffu) + ((b >> 16) & 0xffu) + ((c >> 16) & 0xffu) + ((d >> 16) & 0xffu) + 2u;
      uw |= (su >> 2) << (8 * k);
      vw |= (sv >> 2) << (8 * k);
    }
    const int64_t co = (int64_t)cy * cw + 4 * g;
    store_strip(up + co, uw, nc);
    store_strip(vp + co, vw, nc);
  }
}

}  // namespace

extern "C" int64_t vda_depth_range_workspace(int64_t n) {
  if (n < 1) return 0;
  return ((int64_t)range_grid(n) * 2 * (int64_t)sizeof(float) + 255) / 256 * 256;
}

extern "C" int vda_depth_range(const float* depth, int64_t n, float* range, void* ws, int64_t ws_bytes,
                               void* stream) {
  VDA_CHECK_ARG(depth && range && ws, "null pointer");
  VDA_CHECK_ARG(n >= 1, "depth_range needs n >= 1");
  VDA_CHECK_ARG(((uintptr_t)depth & 3) == 0 && ((uintptr_t)range & 3) == 0 && ((uintptr_t)ws & 3) == 0,
                "depth, range and the workspace must be 4-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_depth_range_workspace(n), "workspace smaller than vda_depth_range_workspace(n)");
  const int grid = range_grid(n);
  float* part = (float*)ws;
  hipLaunchKernelGGL(range_partial_kernel, dim3(grid), dim3(kStreamBlock), 0, (hipStream_t)stream, depth, n, part);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(range_final_kernel, dim3(1), dim3(kStreamBlock), 0, (hipStream_t)stream, (const float*)part, grid,
                     range);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vda_depth_colorize_bytes(int32_t F, int32_t H, int32_t W, int32_t layout) {
  if (F < 1 || H < 1 || W < 1) return 0;
  const int64_t S = (int64_t)H * W;
  switch (layout) {
    case VDA_VIS_INDEX: return F * S;
    case VDA_VIS_HWC:
    case VDA_VIS_PLANAR444: return 3 * F * S;
    case VDA_VIS_PLANAR420: return F * (S + 2 * (int64_t)((H + 1) / 2) * ((W + 1) / 2));
    default: return 0;
  }
}

extern "C" int vda_depth_colorize(const float* depth, int32_t F, int32_t H, int32_t W, const float* range,
                                  const uint8_t* lut, int32_t layout, uint8_t* out, void* stream) {
  VDA_CHECK_ARG(depth && range && out, "null pointer");
  VDA_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "depth_colorize needs F >= 1, H >= 1 and W >= 1");
  VDA_CHECK_ARG(F <= kMaxFrames, "depth_colorize takes F <= 65535 frames per call");
  VDA_CHECK_ARG(layout == VDA_VIS_INDEX || layout == VDA_VIS_HWC || layout == VDA_VIS_PLANAR444 ||
                    layout == VDA_VIS_PLANAR420,
                "unknown layout (VDA_VIS_INDEX, VDA_VIS_HWC, VDA_VIS_PLANAR444 or VDA_VIS_PLANAR420)");
  VDA_CHECK_ARG(lut || layout == VDA_VIS_INDEX, "a layout other than VDA_VIS_INDEX needs a lut");
  VDA_CHECK_ARG(((uintptr_t)depth & 3) == 0 && ((uintptr_t)range & 3) == 0, "depth and range must be 4-byte aligned");
  const int64_t S = (int64_t)H * W;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(color_grid(S), F), block(kStreamBlock);
  switch (layout) {
    case VDA_VIS_INDEX:
      hipLaunchKernelGGL(colorize_kernel<VDA_VIS_INDEX>, grid, block, 0, st, depth, S, range, lut, out);
      break;
    case VDA_VIS_HWC:
      hipLaunchKernelGGL(colorize_kernel<VDA_VIS_HWC>, grid, block, 0, st, depth, S, range, lut, out);
      break;
    case VDA_VIS_PLANAR444:
      hipLaunchKernelGGL(colorize_kernel<VDA_VIS_PLANAR444>, grid, block, 0, st, depth, S, range, lut, out);
      break;
    default:  // a thread takes 16 pixels, so a quarter of the blocks
      hipLaunchKernelGGL(colorize_420_kernel, dim3(color_grid((S + 3) / 4), F), block, 0, st, depth, H, W, range, lut,
                         out);
      break;
  }
  VDA_LAUNCH_CHECK();
  return 0;
}
