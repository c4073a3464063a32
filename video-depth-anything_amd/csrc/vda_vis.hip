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
// Stores are dwords (vda_lut.h): frames and planes start at f * H * W and c * H * W bytes, which are not
// multiples of 4 in general, so every plane is a streaming pass of its own (split by the dword rule on
// the destination): head, body (groups of 4 pixels, one dword per plane, three dwords for interleaved
// RGB) and tail; the depth loads of the body are element-aligned 16-byte loads.  Planes whose heads differ
// (planar 4:4:4 with H * W % 4 != 0) are written in one pass per plane.  4:2:0: a thread owns a strip of
// four 2x2 blocks (8 x 2 pixels): it looks every pixel up once, stores the luma of both rows and the two
// averaged chroma dwords; a strip whose row address is not dword-aligned, or that is cut by the right
// edge, goes out in the widest aligned stores its address allows (bytes and 16-bit words around dwords;
// none of that at W % 8 == 0 with a dword-aligned output).
#include <type_traits>

#include "vda_lut.h"
#include "../../include/vda.h"

namespace {

constexpr int kMaxFrames = 65535;  // grid.y
// range: a block takes 4 16-byte groups per thread while n is large enough; at most 1,024 blocks
int range_grid(int64_t n) { return stream_grid(n, kStreamGroup * 4, 1024); }
// colorize: 4 groups of 4 pixels per thread and pass while the frame is large enough; at most 512 blocks
// per frame
int color_grid(int64_t S) { return stream_grid(S, kStreamGroup * 4, 512); }

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
  block_reduce_ranges(part, nparts, range);
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
  // the packed pixels o .. o + 3 / the pixel e of this frame: the index itself (IDX), or its table row
  // from byte sel0 on
  auto get4 = [&](auto idx, int sel0) {
    return [=](int64_t o, uint32_t (&v)[4]) {
      const f4a4 d = *reinterpret_cast<const f4a4*>(df + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t k = depth_index(d[j], lo, den);
        v[j] = decltype(idx)::value ? k : tab[k] >> (8 * sel0);
      }
    };
  };
  auto get1 = [&](auto idx, int sel0) {
    return [=](int64_t e) {
      const uint32_t k = depth_index(df[e], lo, den);
      return decltype(idx)::value ? k : tab[k] >> (8 * sel0);
    };
  };
  using IdxT = std::true_type;
  using LutT = std::false_type;
  if (LAYOUT == VDA_VIS_INDEX) {
    planes_pass<1>(S, out + f * S, 0, get4(IdxT{}, 0), get1(IdxT{}, 0));
  } else if (LAYOUT == VDA_VIS_HWC) {
    hwc_pass(S, out + 3 * f * S, get4(LutT{}, 0), get1(LutT{}, 0));  // the top byte is 0
  } else {
    uint8_t* of = out + 3 * f * S;
    if ((S & 3) == 0) {  // the three planes share their alignment: one pass
      planes_pass<3>(S, of, S, get4(LutT{}, 0), get1(LutT{}, 0));
    } else {
      for (int c = 0; c < 3; ++c) planes_pass<1>(S, of + c * S, 0, get4(LutT{}, c), get1(LutT{}, c));
    }
  }
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
    const int64_t co = (int64_t)cy * cw + 4 * g;
    store_strip_420(v, yp + (int64_t)y0 * W + x0, W, two, nv, up + co, vp + co, nc);
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
