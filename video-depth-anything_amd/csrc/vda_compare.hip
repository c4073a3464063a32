// The ground-truth comparison video on the device (the reference's utils/vis_util.py: visualise_data): the
// range of the error maps, and per output frame a canvas of tiles (RGB frame, GT depth, per method an error
// map, the prediction and an x-t "stability" slice) straight to the bytes of the output file.  The contract,
// the tile kinds and the deviations from the reference's matplotlib figure are in include/vda.h.
//
// absdiff_range: vda_depth_range's two-stage min / max (vda_stream.h) over e = valid ? |gt - pred| : 0: the
//           split is pred's, gt and valid share its head and are read with element-aligned vector loads.
//           HBM-bound: 8 B per element read (9 B with a mask).
// compose:  a canvas frame is one flat run of rows * H * cols * W pixels and goes out through the passes of
//           vda_lut.h (planes, interleaved rows, 4:2:0 strips); what differs from vda_depth_colorize is
//           where a pixel comes from.  A block stages the (at most 12) grid cells once in LDS: kind,
//           operand pointers, frame offset and the range as (lo, den), and the two colour tables as packed
//           dwords.  A group of 4 (a strip of 8) canvas pixels that lies within one tile row, which is every
//           group but those at the tile seams, reads its cell once and its float operands with 16-byte
//           loads; a group across a seam or a row end is evaluated pixel by pixel.  Per canvas pixel of a
//           tile column of M = 1 (RGB over error map, GT over prediction, two x-t slices): 3 + 8 B, 4 + 4 B
//           and 2 x 4 B read (the x-t reads are one column, strided), 18 B written (9 B at 4:2:0).
#include "vda_lut.h"
#include "../../include/vda.h"

namespace {

constexpr int kMaxFrames = 65535;  // grid.y
constexpr int kMaxTiles = 12, kMaxRows = 4, kMaxCols = 3;
constexpr int kNone = -1;  // a cell without a tile
int range_grid(int64_t n) { return stream_grid(n, kStreamGroup * 4, 1024); }
int canvas_grid(int64_t S) { return stream_grid(S, kStreamGroup * 4, 512); }

template <bool MASK>
__global__ __launch_bounds__(kStreamBlock) void absdiff_partial_kernel(const float* __restrict__ a,
                                                                       const float* __restrict__ b,
                                                                       const uint8_t* __restrict__ valid, int64_t n,
                                                                       float* __restrict__ part) {
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const StreamSplit sp = stream_split_f32(a, n);
  stream_walk(
      n, sp.head, sp.nvec,
      [&](int64_t o) {
        const f4 p = *reinterpret_cast<const f4*>(a + o);
        const f4a4 g = *reinterpret_cast<const f4a4*>(b + o);
        u8x4a1 m = {1, 1, 1, 1};
        if (MASK) m = *reinterpret_cast<const u8x4a1*>(valid + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float e = m[j] ? fabsf(g[j] - p[j]) : 0.f;
          mn = fminf(mn, e);
          mx = fmaxf(mx, e);
        }
      },
      [&](int64_t i) {
        const float e = (!MASK || valid[i]) ? fabsf(b[i] - a[i]) : 0.f;
        mn = fminf(mn, e);
        mx = fmaxf(mx, e);
      });
  block_store_range(mn, mx, part + 2 * (int64_t)blockIdx.x);
}

__global__ __launch_bounds__(kStreamBlock) void absdiff_final_kernel(const float* __restrict__ part, int nparts,
                                                                     float* __restrict__ range) {
  block_reduce_ranges(part, nparts, range);
}

// ---- the canvas --------------------------------------------------------------------------------
struct PanelArgs {
  vda_tile tile[kMaxTiles];
  int32_t ntiles, cols;
  int32_t t0, N, H, W, xstar;
  const uint8_t* lut0;
  const uint8_t* lut1;
  uint8_t* out;
};

// A grid cell as the pixels need it (LDS).
struct Cell {
  const uint8_t* a;
  const float* b;
  const uint8_t* valid;
  float lo, den;
  int32_t kind, o, n, lut;
};

struct Geo {
  int32_t H, W, CH, CW;  // tile and canvas size
  int64_t S;             // H * W
  int32_t N, xstar, t;
  bool yuv, xt32;        // planar layout: RGB tiles are converted; W * N fits 32 bits
  uint32_t black;
};

__device__ __forceinline__ uint32_t quant8(float x) {
  const float r = rintf(x);
  return r >= 255.f ? 255u : (r > 0.f ? (uint32_t)(int)r : 0u);
}

// video_io._rgb_to_yuv operation for operation (include/vda.h), packed Y | U << 8 | V << 16.
__device__ __forceinline__ uint32_t rgb_to_yuv601(uint32_t r8, uint32_t g8, uint32_t b8) {
#pragma clang fp contract(off)
  const float r = (float)r8, g = (float)g8, b = (float)b8;
  const float y = (0.299f * r + 0.587f * g) + 0.114f * b;
  const float u = (b - y) / 1.772f;
  const float v = (r - y) / 1.402f;
  const float ky = (float)(219.0 / 255.0), kc = (float)(224.0 / 255.0);
  return quant8(y * ky + 16.0f) | (quant8(u * kc + 128.0f) << 8) | (quant8(v * kc + 128.0f) << 16);
}

template <int K>
__device__ __forceinline__ void load_run(const float* __restrict__ p, float (&d)[K]) {
  if constexpr (K % 4 == 0) {
#pragma unroll
    for (int h = 0; h < K / 4; ++h) {
      const f4a4 q = *reinterpret_cast<const f4a4*>(p + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * h + j] = q[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = p[j];
  }
}

template <int K>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ p, uint32_t (&d)[K]) {
  if constexpr (K % 4 == 0) {
#pragma unroll
    for (int h = 0; h < K / 4; ++h) {
      const u8x4a1 q = *reinterpret_cast<const u8x4a1*>(p + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * h + j] = q[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = p[j];
  }
}

// The K packed pixels (y, px .. px + K - 1) of one tile row; px + K <= W.
template <int K>
__device__ __forceinline__ void cell_run(const Cell& ce, const uint32_t* tab, const Geo& g, int y, int px,
                                         uint32_t (&v)[K]) {
  const int kind = ce.kind;
  const int s = g.t - ce.o;
  const bool live = s >= 0 && s < ce.n;
  if (kind == kNone || (kind == VDA_TILE_RGB && !live)) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = g.black;
    return;
  }
  const int64_t row = (int64_t)y * g.W;
  const int64_t e = (int64_t)s * g.S + row + px;  // used when live
  if (kind == VDA_TILE_RGB) {
    uint32_t c[3 * K];
    load_run<3 * K>(ce.a + 3 * e, c);
#pragma unroll
    for (int j = 0; j < K; ++j)
      v[j] = g.yuv ? rgb_to_yuv601(c[3 * j], c[3 * j + 1], c[3 * j + 2])
                   : c[3 * j] | (c[3 * j + 1] << 8) | (c[3 * j + 2] << 16);
    return;
  }
  float d[K];
  if (kind == VDA_TILE_XT) {
    const float* src = reinterpret_cast<const float*>(ce.a) + row + g.xstar;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int c = g.xt32 ? (int)((uint32_t)(px + j) * (uint32_t)g.N / (uint32_t)g.W)
                           : (int)((uint64_t)(px + j) * (uint64_t)g.N / (uint64_t)g.W);
      const int sc = c - ce.o;
      d[j] = (c <= g.t && sc >= 0 && sc < ce.n) ? src[(int64_t)sc * g.S] : 0.f;
    }
  } else if (!live) {
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = 0.f;
  } else {
    load_run<K>(reinterpret_cast<const float*>(ce.a) + e, d);
    if (kind == VDA_TILE_ERROR) {
      float gt[K];
      load_run<K>(ce.b + e, gt);
#pragma unroll
      for (int j = 0; j < K; ++j) d[j] = fabsf(gt[j] - d[j]);
      if (ce.valid) {
        uint32_t m[K];
        load_run<K>(ce.valid + e, m);
#pragma unroll
        for (int j = 0; j < K; ++j) d[j] = m[j] ? d[j] : 0.f;
      }
    }
  }
  const uint32_t* tb = tab + 256 * ce.lut;
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = tb[depth_index(d[j], ce.lo, ce.den)];
}

struct Canvas {
  const Cell* cells;  // [kMaxRows * kMaxCols], cell (r, c) at r * kMaxCols + c
  const uint32_t* tab;
  Geo g;

  __device__ __forceinline__ int tile_col(int X) const { return (X >= g.W) + (X >= 2 * g.W); }
  __device__ __forceinline__ int tile_row(int Y) const { return (Y >= g.H) + (Y >= 2 * g.H) + (Y >= 3 * g.H); }

  // The canvas pixels (Y, X .. X + K - 1), all within tile column c.
  template <int K>
  __device__ __forceinline__ void run(int Y, int X, int c, uint32_t (&v)[K]) const {
    const int r = tile_row(Y);
    cell_run<K>(cells[r * kMaxCols + c], tab, g, Y - r * g.H, X - c * g.W, v);
  }
  __device__ __forceinline__ uint32_t pixel(int Y, int X) const {
    uint32_t v[1];
    run<1>(Y, X, tile_col(X), v);
    return v[0];
  }
  // The pixels p .. p + 3 of the canvas as a flat run.
  __device__ __forceinline__ void flat4(int64_t p, uint32_t (&v)[4]) const {
    int Y = (int)((uint32_t)p / (uint32_t)g.CW);
    int X = (int)((uint32_t)p - (uint32_t)Y * (uint32_t)g.CW);
    const int c = tile_col(X);
    if (X + 3 < g.CW && tile_col(X + 3) == c) {
      run<4>(Y, X, c, v);
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = pixel(Y, X);
      if (++X == g.CW) X = 0, ++Y;
    }
  }
  __device__ __forceinline__ uint32_t flat1(int64_t p) const {
    const int Y = (int)((uint32_t)p / (uint32_t)g.CW);
    return pixel(Y, (int)((uint32_t)p - (uint32_t)Y * (uint32_t)g.CW));
  }
};

// The cells and the two tables of a block.  Thread i stages tile i: the loop is unrolled, so the kernel
// arguments are read at constant offsets.
__device__ __forceinline__ void stage_canvas(const PanelArgs& A, Cell* cells, uint32_t* tab) {
  if (threadIdx.x < kMaxRows * kMaxCols) cells[threadIdx.x].kind = kNone;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kMaxTiles; ++i) {
    if (i < A.ntiles && (int)threadIdx.x == i) {
      const vda_tile& t = A.tile[i];
      Cell c;
      c.a = reinterpret_cast<const uint8_t*>(t.a);
      c.b = t.b;
      c.valid = t.valid;
      c.lo = 0.f, c.den = 1.f;
      if (t.kind != VDA_TILE_RGB) {
        c.lo = t.range[0];
        c.den = t.range[1] - c.lo;
      }
      c.kind = t.kind, c.o = t.offset, c.n = t.frames, c.lut = t.lut;
      cells[t.row * kMaxCols + t.col] = c;
    }
  }
  if (A.lut0) stage_table(A.lut0, tab);
  if (A.lut1) stage_table(A.lut1, tab + 256);
  __syncthreads();
}

__device__ __forceinline__ Canvas make_canvas(const PanelArgs& A, int rows, int layout, const Cell* cells,
                                              const uint32_t* tab) {
  Canvas cv;
  cv.cells = cells, cv.tab = tab;
  Geo& g = cv.g;
  g.H = A.H, g.W = A.W, g.CH = rows * A.H, g.CW = A.cols * A.W;
  g.S = (int64_t)A.H * A.W;
  g.N = A.N, g.xstar = A.xstar, g.t = A.t0 + (int)blockIdx.y;
  g.yuv = layout != VDA_VIS_HWC;
  g.xt32 = (uint64_t)A.W * (uint64_t)A.N <= 0xffffffffull;
  g.black = g.yuv ? (16u | (128u << 8) | (128u << 16)) : 0u;
  return cv;
}

// Canvas frame f = blockIdx.y; its pixels are spread over gridDim.x blocks.
template <int LAYOUT>
__global__ __launch_bounds__(kStreamBlock) void compose_kernel(const PanelArgs A, int rows) {
  __shared__ Cell cells[kMaxRows * kMaxCols];
  __shared__ uint32_t tab[512];
  stage_canvas(A, cells, tab);
  const Canvas cv = make_canvas(A, rows, LAYOUT, cells, tab);
  const int64_t Sc = (int64_t)cv.g.CH * cv.g.CW;
  uint8_t* of = A.out + 3 * (int64_t)blockIdx.y * Sc;
  auto get4 = [&](int sel0) { return [&cv, sel0](int64_t o, uint32_t (&v)[4]) {
    cv.flat4(o, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] >>= 8 * sel0;
  }; };
  auto get1 = [&](int sel0) { return [&cv, sel0](int64_t e) { return cv.flat1(e) >> (8 * sel0); }; };
  if (LAYOUT == VDA_VIS_HWC) {
    hwc_pass(Sc, of, get4(0), get1(0));
  } else if ((Sc & 3) == 0) {  // the three planes share their alignment: one pass
    planes_pass<3>(Sc, of, Sc, get4(0), get1(0));
  } else {
    for (int c = 0; c < 3; ++c) planes_pass<1>(Sc, of + c * Sc, 0, get4(c), get1(c));
  }
}

// 4:2:0: the strips of vda_depth_colorize's kernel over the canvas: unit u is chroma row cy = u / ns, chroma
// columns 4 g .. 4 g + 3, canvas pixels [2 cy, 2 cy + 1] x [8 g, 8 g + 7], rows and columns past the canvas
// edge repeating the last one.
__global__ __launch_bounds__(kStreamBlock) void compose_420_kernel(const PanelArgs A, int rows) {
  __shared__ Cell cells[kMaxRows * kMaxCols];
  __shared__ uint32_t tab[512];
  stage_canvas(A, cells, tab);
  const Canvas cv = make_canvas(A, rows, VDA_VIS_PLANAR420, cells, tab);
  const int CH = cv.g.CH, CW = cv.g.CW;
  const int64_t Sc = (int64_t)CH * CW;
  const int ch = (CH + 1) / 2, cw = (CW + 1) / 2;
  const int64_t C = (int64_t)ch * cw;
  uint8_t* yp = A.out + (int64_t)blockIdx.y * (Sc + 2 * C);
  uint8_t* up = yp + Sc;
  uint8_t* vp = up + C;
  const int64_t ns = (cw + 3) / 4;
  const int64_t units = (int64_t)ch * ns;
  const int64_t stride = (int64_t)gridDim.x * kStreamBlock;
  for (int64_t u = (int64_t)blockIdx.x * kStreamBlock + threadIdx.x; u < units; u += stride) {
    const int cy = (int)(u / ns);
    const int g = (int)(u - (int64_t)cy * ns);
    const int x0 = 8 * g, y0 = 2 * cy;
    const bool two = y0 + 1 < CH;
    const int y1 = two ? y0 + 1 : y0;
    const int nv = CW - x0 < 8 ? CW - x0 : 8;        // luma bytes of the strip per row, 1..8
    const int nc = cw - 4 * g < 4 ? cw - 4 * g : 4;  // chroma bytes of the strip per plane, 1..4
    uint32_t v[2][8];
    const int c = cv.tile_col(x0);
    if (nv == 8 && cv.tile_col(x0 + 7) == c) {
      cv.run<8>(y0, x0, c, v[0]);
      cv.run<8>(y1, x0, c, v[1]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = x0 + (j < nv ? j : nv - 1);
        v[0][j] = cv.pixel(y0, x);
        v[1][j] = cv.pixel(y1, x);
      }
    }
    const int64_t co = (int64_t)cy * cw + 4 * g;
    store_strip_420(v, yp + (int64_t)y0 * CW + x0, CW, two, nv, up + co, vp + co, nc);
  }
}

}  // namespace

extern "C" int64_t vda_tile_size(void) { return (int64_t)sizeof(vda_tile); }

extern "C" int64_t vda_depth_absdiff_range_workspace(int64_t n) {
  if (n < 1) return 0;
  return ((int64_t)range_grid(n) * 2 * (int64_t)sizeof(float) + 255) / 256 * 256;
}

extern "C" int vda_depth_absdiff_range(const float* a, const float* b, const uint8_t* valid, int64_t n, float* range,
                                       void* ws, int64_t ws_bytes, void* stream) {
  VDA_CHECK_ARG(a && b && range && ws, "null pointer");
  VDA_CHECK_ARG(n >= 1, "depth_absdiff_range needs n >= 1");
  VDA_CHECK_ARG(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 && ((uintptr_t)range & 3) == 0 &&
                    ((uintptr_t)ws & 3) == 0,
                "a, b, range and the workspace must be 4-byte aligned");
  VDA_CHECK_ARG(ws_bytes >= vda_depth_absdiff_range_workspace(n),
                "workspace smaller than vda_depth_absdiff_range_workspace(n)");
  const int grid = range_grid(n);
  float* part = (float*)ws;
  if (valid)
    hipLaunchKernelGGL(absdiff_partial_kernel<true>, dim3(grid), dim3(kStreamBlock), 0, (hipStream_t)stream, a, b, valid,
                       n, part);
  else
    hipLaunchKernelGGL(absdiff_partial_kernel<false>, dim3(grid), dim3(kStreamBlock), 0, (hipStream_t)stream, a, b, valid,
                       n, part);
  VDA_LAUNCH_CHECK();
  hipLaunchKernelGGL(absdiff_final_kernel, dim3(1), dim3(kStreamBlock), 0, (hipStream_t)stream, (const float*)part, grid,
                     range);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vda_panel_compose_bytes(int32_t F, int32_t rows, int32_t cols, int32_t H, int32_t W,
                                           int32_t layout) {
  if (F < 1 || rows < 1 || cols < 1 || H < 1 || W < 1) return 0;
  const int64_t CH = (int64_t)rows * H, CW = (int64_t)cols * W;
  switch (layout) {
    case VDA_VIS_HWC:
    case VDA_VIS_PLANAR444: return 3 * F * CH * CW;
    case VDA_VIS_PLANAR420: return F * (CH * CW + 2 * ((CH + 1) / 2) * ((CW + 1) / 2));
    default: return 0;
  }
}

extern "C" int vda_panel_compose(const vda_tile* tiles, int32_t ntiles, int32_t rows, int32_t cols, int32_t F,
                                 int32_t t0, int32_t N, int32_t H, int32_t W, int32_t xstar, const uint8_t* lut0,
                                 const uint8_t* lut1, int32_t layout, uint8_t* out, void* stream) {
  VDA_CHECK_ARG(tiles && out, "null pointer");
  VDA_CHECK_ARG(ntiles >= 1 && ntiles <= kMaxTiles, "panel_compose takes 1 to 12 tiles");
  VDA_CHECK_ARG(rows >= 1 && rows <= kMaxRows && cols >= 1 && cols <= kMaxCols,
                "panel_compose needs a grid of 1..4 rows by 1..3 columns");
  VDA_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && N >= 1, "panel_compose needs F >= 1, N >= 1, H >= 1 and W >= 1");
  VDA_CHECK_ARG(F <= kMaxFrames, "panel_compose takes F <= 65535 frames per call");
  VDA_CHECK_ARG(t0 >= 0 && (int64_t)t0 + F <= N, "panel_compose needs 0 <= t0 and t0 + F <= N");
  VDA_CHECK_ARG(xstar >= 0 && xstar < W, "panel_compose needs 0 <= xstar < W");
  VDA_CHECK_ARG(layout == VDA_VIS_HWC || layout == VDA_VIS_PLANAR444 || layout == VDA_VIS_PLANAR420,
                "unknown layout (VDA_VIS_HWC, VDA_VIS_PLANAR444 or VDA_VIS_PLANAR420)");
  VDA_CHECK_ARG(H < (1 << 28) && W < (1 << 28) && (int64_t)rows * H * cols * W < (1ll << 31),
                "the canvas must hold fewer than 2^31 pixels");
  PanelArgs A;
  bool taken[kMaxRows * kMaxCols] = {};
  for (int i = 0; i < kMaxTiles; ++i) A.tile[i] = vda_tile{};
  for (int i = 0; i < ntiles; ++i) {
    const vda_tile& t = tiles[i];
    VDA_CHECK_ARG(t.kind >= VDA_TILE_RGB && t.kind <= VDA_TILE_XT,
                  "unknown tile kind (VDA_TILE_RGB, VDA_TILE_DEPTH, VDA_TILE_ERROR or VDA_TILE_XT)");
    VDA_CHECK_ARG(t.row >= 0 && t.row < rows && t.col >= 0 && t.col < cols, "a tile lies outside the grid");
    VDA_CHECK_ARG(!taken[t.row * kMaxCols + t.col], "two tiles share a grid cell");
    taken[t.row * kMaxCols + t.col] = true;
    VDA_CHECK_ARG(t.a, "a tile without a source (null pointer)");
    VDA_CHECK_ARG(t.offset >= 0 && t.frames >= 1, "a tile needs offset >= 0 and frames >= 1");
    if (t.kind != VDA_TILE_RGB) {
      VDA_CHECK_ARG(t.range, "a depth, error or x-t tile needs a range (null pointer)");
      VDA_CHECK_ARG(t.lut == 0 || t.lut == 1, "a tile's lut must be 0 or 1");
      VDA_CHECK_ARG(t.lut == 0 ? lut0 != nullptr : lut1 != nullptr, "a tile names a lut that is NULL");
      VDA_CHECK_ARG(((uintptr_t)t.a & 3) == 0 && ((uintptr_t)t.range & 3) == 0,
                    "float sources and ranges must be 4-byte aligned");
    }
    if (t.kind == VDA_TILE_ERROR)
      VDA_CHECK_ARG(t.b && ((uintptr_t)t.b & 3) == 0, "an error tile needs a 4-byte-aligned second operand");
    A.tile[i] = t;
  }
  A.ntiles = ntiles, A.cols = cols, A.t0 = t0, A.N = N, A.H = H, A.W = W, A.xstar = xstar;
  A.lut0 = lut0, A.lut1 = lut1, A.out = out;
  const int64_t Sc = (int64_t)rows * H * cols * W;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(canvas_grid(Sc), F), block(kStreamBlock);
  switch (layout) {
    case VDA_VIS_HWC: hipLaunchKernelGGL(compose_kernel<VDA_VIS_HWC>, grid, block, 0, st, A, rows); break;
    case VDA_VIS_PLANAR444: hipLaunchKernelGGL(compose_kernel<VDA_VIS_PLANAR444>, grid, block, 0, st, A, rows); break;
    default:  // a thread takes 16 pixels, so a quarter of the blocks
      hipLaunchKernelGGL(compose_420_kernel, dim3(canvas_grid((Sc + 3) / 4), F), block, 0, st, A, rows);
      break;
  }
  VDA_LAUNCH_CHECK();
  return 0;
}
