// Planar YUV frames (the payload of a YUV4MPEG2 file, as it lies in the file) to RGB and to the network input.
//
// A frame is frame_stride bytes apart from the next and holds the Y plane (h * w bytes), then U, then V
// (ch * cw bytes each; 4:2:0 cw = (w+1)/2, ch = (h+1)/2; 4:2:2 cw = (w+1)/2, ch = h; 4:4:4 cw = w, ch = h;
// mono none, u = v = 128).  Chroma is taken nearest (u[y >> sy][x >> sx]) and the pixel converted BT.601
// limited range -> RGB in fp32, every operation rounded once (no contraction), round half to even, clamp:
// video_io._yuv_to_rgb as numpy float32 computes it, bit for bit.
//
// yuv_to_rgb:     uint8 [N, h, w, 3]; a thread takes 4 pixels of a row: one dword of Y, a 16-bit word (or a
//                 dword) per chroma plane, three dwords out - each only where its address allows, bytes
//                 otherwise (src has no alignment: planes and rows are misaligned whenever h * w is odd).
// preprocess_yuv: float [N, 3, H, W] = vda_preprocess_frames of those RGB frames, bit for bit: both kernels
//                 instantiate vda_pre::preprocess_pixel (vda_preprocess.h).  A workgroup owns kTileW x kTileH
//                 output pixels, converts the clamped source footprint of that tile once into LDS (per pixel
//                 the three channels already divided by 255, one plane per channel; staged in units of 4
//                 pixels: dword / word loads where the address allows, one 16-byte LDS store per plane) and
//                 interpolates from there, 4 outputs per thread, consecutive lanes on consecutive output
//                 columns.  The 48 divisions by 255 an output pixel takes in the RGB kernel are made once per
//                 source pixel here.  The footprint of a tile grows with the downscale ratio; when its bound
//                 exceeds kCapPx the entry point runs yuv_to_rgb into the caller's workspace and
//                 vda_preprocess_frames on that (vda_preprocess_yuv_workspace > 0).
// yuv_downscale:  uint8 [N, h2, w2, 3] = Pillow's Image.resize((w2, h2), BICUBIC) of those RGB frames, bit for
//                 bit: ImagingResample's 8-bit path is integer fixed point (22 fractional bits), horizontal pass,
//                 uint8, vertical pass, from coefficient tables the host builds in doubles (vda_resample_tables).
//                 A workgroup owns kDsTileW x kDsTileH output pixels: it converts the source rows of the tile's
//                 footprint kDsChunk at a time into LDS (one packed word per pixel), filters them horizontally
//                 into LDS, filters those vertically and stores the tile's rows as runs of dwords.  Neither the
//                 full-size RGB frame nor the horizontal intermediate reaches memory.  Where w % 4 == 0 and the
//                 frames are dword-aligned the rows are staged with branch-free wide loads, two units of 4
//                 pixels in flight per thread; every other layout goes through convert4_any.
#include "vda_preprocess.h"
#include "../../include/vda.h"

namespace {

using vda_pre::NormArgs;

constexpr int kBlock = 256;
constexpr int kTileW = 64;            // output columns of a tile = lanes of a wave
constexpr int kTileH = 16;            // output rows of a tile: kBlock / kTileW waves x kRowsPerThread
constexpr int kRowsPerThread = kTileH / (kBlock / kTileW);
constexpr int kCapPx = 3072;          // footprint capacity in pixels (3 float planes: 36 KiB of LDS)
constexpr int kMaxGridYZ = 65535;

typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));

struct Planes {
  int cw, ch;   // chroma plane size (0: mono)
  int sx, sy;   // chroma shifts
};

__host__ __device__ inline Planes planes_of(int h, int w, int chroma) {
  Planes p;
  p.sx = (chroma == VDA_YUV_420 || chroma == VDA_YUV_422) ? 1 : 0;
  p.sy = chroma == VDA_YUV_420 ? 1 : 0;
  p.cw = chroma == VDA_YUV_MONO ? 0 : (w + p.sx) >> p.sx;
  p.ch = chroma == VDA_YUV_MONO ? 0 : (h + p.sy) >> p.sy;
  return p;
}

int64_t payload_bytes(int h, int w, int chroma) {
  const Planes p = planes_of(h, w, chroma);
  return (int64_t)h * w + 2 * (int64_t)p.cw * p.ch;
}

// video_io._yuv_to_rgb for one pixel -> r | g << 8 | b << 16.  The constants are the float32 roundings of the
// Python doubles numpy multiplies its float32 arrays by.
__device__ __forceinline__ uint32_t yuv_pixel(uint32_t y, uint32_t u, uint32_t v) {
#pragma clang fp contract(off)
  const float ky = (float)(255.0 / 219.0), kc = (float)(255.0 / 224.0);
  const float yf = ((float)y - 16.0f) * ky;
  const float uf = ((float)u - 128.0f) * kc;
  const float vf = ((float)v - 128.0f) * kc;
  const float rv = 1.402f * vf;
  const float gu = 0.344136f * uf;
  const float gv = 0.714136f * vf;
  const float bu = 1.772f * uf;
  const float r = yf + rv;
  const float g = (yf - gu) - gv;
  const float b = yf + bu;
  const uint32_t ri = (uint32_t)(int)fminf(fmaxf(rintf(r), 0.f), 255.f);
  const uint32_t gi = (uint32_t)(int)fminf(fmaxf(rintf(g), 0.f), 255.f);
  const uint32_t bi = (uint32_t)(int)fminf(fmaxf(rintf(b), 0.f), 255.f);
  return ri | (gi << 8) | (bi << 16);
}

// Pixels x0 .. x0 + 3 (x0 % 4 == 0) of row y of one frame, converted; pixels at x >= w give 0 and nothing
// beyond the row's last byte is read.  yrow = Y plane row y, urow / vrow = chroma row y >> sy (unused for mono).
template <int SX, bool MONO>
__device__ __forceinline__ void convert4(const uint8_t* __restrict__ yrow, const uint8_t* __restrict__ urow,
                                         const uint8_t* __restrict__ vrow, int w, int cw, int x0, uint32_t px[4]) {
  const int n = w - x0 < 4 ? w - x0 : 4;  // valid pixels, >= 1
  uint32_t yy[4], uu[4], vv[4];
  const uint8_t* py = yrow + x0;
  if (n == 4 && ((uintptr_t)py & 3) == 0) {
    const uint32_t d = *reinterpret_cast<const uint32_t*>(py);
#pragma unroll
    for (int j = 0; j < 4; ++j) yy[j] = (d >> (8 * j)) & 0xffu;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) yy[j] = j < n ? py[j] : 0u;
  }
  if (MONO) {
#pragma unroll
    for (int j = 0; j < 4; ++j) uu[j] = vv[j] = 128u;
  } else if (SX == 1) {
    const int c0 = x0 >> 1;
    const uint8_t* pu = urow + c0;
    const uint8_t* pv = vrow + c0;
    const bool two = c0 + 1 < cw;  // n >= 3 needs the second chroma sample, and then it exists
    uint32_t a[2], b[2];
    if (two && ((uintptr_t)pu & 1) == 0) {
      const uint32_t d = *reinterpret_cast<const uint16_t*>(pu);
      a[0] = d & 0xffu, a[1] = d >> 8;
    } else {
      a[0] = pu[0], a[1] = two ? pu[1] : 0u;
    }
    if (two && ((uintptr_t)pv & 1) == 0) {
      const uint32_t d = *reinterpret_cast<const uint16_t*>(pv);
      b[0] = d & 0xffu, b[1] = d >> 8;
    } else {
      b[0] = pv[0], b[1] = two ? pv[1] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) uu[j] = a[j >> 1], vv[j] = b[j >> 1];
  } else {
    const uint8_t* pu = urow + x0;
    const uint8_t* pv = vrow + x0;
    if (n == 4 && ((uintptr_t)pu & 3) == 0) {
      const uint32_t d = *reinterpret_cast<const uint32_t*>(pu);
#pragma unroll
      for (int j = 0; j < 4; ++j) uu[j] = (d >> (8 * j)) & 0xffu;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) uu[j] = j < n ? pu[j] : 0u;
    }
    if (n == 4 && ((uintptr_t)pv & 3) == 0) {
      const uint32_t d = *reinterpret_cast<const uint32_t*>(pv);
#pragma unroll
      for (int j = 0; j < 4; ++j) vv[j] = (d >> (8 * j)) & 0xffu;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) vv[j] = j < n ? pv[j] : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) px[j] = j < n ? yuv_pixel(yy[j], uu[j], vv[j]) : 0u;
}

__device__ __forceinline__ void convert4_any(int chroma, const uint8_t* __restrict__ frame, int h, int w,
                                             const Planes& pl, int y, int x0, uint32_t px[4]) {
  const uint8_t* yrow = frame + (size_t)y * w;
  const size_t csz = (size_t)pl.cw * pl.ch;
  const uint8_t* urow = frame + (size_t)h * w + (size_t)(y >> pl.sy) * pl.cw;
  const uint8_t* vrow = urow + csz;
  if (chroma == VDA_YUV_MONO) convert4<0, true>(yrow, yrow, yrow, w, 0, x0, px);
  else if (pl.sx) convert4<1, false>(yrow, urow, vrow, w, pl.cw, x0, px);
  else convert4<0, false>(yrow, urow, vrow, w, pl.cw, x0, px);
}

// grid (ceil(ceil(w / 4) / kBlock), h, N): a thread converts 4 pixels of row blockIdx.y.
__global__ __launch_bounds__(kBlock) void yuv_to_rgb_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            int h, int w, int64_t frame_stride, int chroma) {
  const int x0 = 4 * (blockIdx.x * kBlock + threadIdx.x);
  const int y = blockIdx.y;
  const int n = blockIdx.z;
  if (x0 >= w) return;
  const Planes pl = planes_of(h, w, chroma);
  uint32_t px[4];
  convert4_any(chroma, src + (size_t)n * frame_stride, h, w, pl, y, x0, px);
  uint8_t* o = dst + (((size_t)n * h + y) * w + x0) * 3;
  const int cnt = w - x0 < 4 ? w - x0 : 4;
  if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
    u32x3a4 v;
    v[0] = px[0] | (px[1] << 24);
    v[1] = (px[1] >> 8) | (px[2] << 16);
    v[2] = (px[2] >> 16) | (px[3] << 8);
    *reinterpret_cast<u32x3a4*>(o) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        o[3 * j] = (uint8_t)px[j];
        o[3 * j + 1] = (uint8_t)(px[j] >> 8);
        o[3 * j + 2] = (uint8_t)(px[j] >> 16);
      }
    }
  }
}

// Source pixel (y, x) of the staged footprint: rows y0 .. y0 + fh - 1, columns x0 .. x0 + pitch - 1.  The
// coordinates preprocess_pixel asks for lie inside it by construction (the footprint's corners come from the
// same src_coord); the clamp keeps the LDS index in range whatever the compiler made of the two call sites.
struct LdsFetch {
  const float* tile;  // [3][kCapPx]
  int y0, x0, fh, pitch;
  __device__ __forceinline__ vda_pre::Px operator()(int y, int x) const {
    const int ly = min(max(y - y0, 0), fh - 1);
    const int lx = min(max(x - x0, 0), pitch - 1);
    const int i = ly * pitch + lx;
    return {{tile[i], tile[kCapPx + i], tile[2 * kCapPx + i]}};
  }
};

// grid (ceil(W / kTileW), ceil(H / kTileH), N)
__global__ __launch_bounds__(kBlock) void preprocess_yuv_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                                int h, int w, int64_t frame_stride, int chroma,
                                                                int H, int W, NormArgs na) {
  __shared__ __attribute__((aligned(16))) float tile[3 * kCapPx];
  const int ox0 = blockIdx.x * kTileW, oy0 = blockIdx.y * kTileH;
  const int ox1 = min(ox0 + kTileW, W) - 1, oy1 = min(oy0 + kTileH, H) - 1;
  const int n = blockIdx.z;
  // the clamped 4-tap window of the tile's first and last output row / column; columns start at a multiple of 4
  const int ya = min(max((int)floorf(vda_pre::src_coord(h, H, oy0)) - 1, 0), h - 1);
  const int yb = min(max((int)floorf(vda_pre::src_coord(h, H, oy1)) + 2, 0), h - 1);
  const int xa = min(max((int)floorf(vda_pre::src_coord(w, W, ox0)) - 1, 0), w - 1) & ~3;
  const int xb = min(max((int)floorf(vda_pre::src_coord(w, W, ox1)) + 2, 0), w - 1);
  const int upr = (xb - xa) / 4 + 1;  // units of 4 pixels per footprint row
  const int pitch = 4 * upr;
  int fh = yb - ya + 1;
  if (fh * pitch > kCapPx) fh = kCapPx / pitch;  // never: the entry point routes by a bound on fh * pitch
  const Planes pl = planes_of(h, w, chroma);
  const uint8_t* frame = src + (size_t)n * frame_stride;
  for (int u = threadIdx.x; u < fh * upr; u += kBlock) {
    const int ly = u / upr, q = u - ly * upr;
    uint32_t px[4];
    convert4_any(chroma, frame, h, w, pl, ya + ly, xa + 4 * q, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = vda_pre::unit_scale((px[j] >> (8 * c)) & 0xffu);
      *reinterpret_cast<f4*>(&tile[c * kCapPx + ly * pitch + 4 * q]) = v;
    }
  }
  __syncthreads();
  const LdsFetch fetch{tile, ya, xa, fh, pitch};
  const int ox = ox0 + (threadIdx.x & (kTileW - 1));
  if (ox >= W) return;
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int oy = oy0 + (threadIdx.x / kTileW) + j * (kBlock / kTileW);
    if (oy < H)
      vda_pre::preprocess_pixel(fetch, h, w, H, W, oy, ox, na, dst + (size_t)n * 3 * plane + (size_t)oy * W + ox, plane);
  }
}

// Upper bound of a tile's staged footprint in pixels: kTileW output columns span at most ceil((kTileW - 1) * w / W)
// source columns, + 1 for the rounding of the two corner coordinates, + 3 for the 4-tap window, + 3 for the
// start moved down to a multiple of 4, rounded up to whole units; rows alike without the unit terms.
int64_t footprint_bound(int h, int w, int H, int W) {
  int64_t fw = ((int64_t)(kTileW - 1) * w + W - 1) / W + 1 + 1 + 3 + 3;
  fw = (fw + 3) / 4 * 4;
  const int64_t wcap = ((int64_t)w + 3) / 4 * 4;
  if (fw > wcap) fw = wcap;
  int64_t fh = ((int64_t)(kTileH - 1) * h + H - 1) / H + 1 + 1 + 3;
  if (fh > h) fh = h;
  return fw * fh;
}

bool chroma_ok(int c) { return c == VDA_YUV_420 || c == VDA_YUV_422 || c == VDA_YUV_444 || c == VDA_YUV_MONO; }

// ---- yuv_downscale: Pillow's antialiased bicubic resize of the decoded frames, in its integer arithmetic ----
constexpr int kDsTileW = 64;      // output columns of a tile = lanes of a wave
constexpr int kDsTileH = 16;      // output rows of a tile
constexpr int kDsWaves = kBlock / 64;
constexpr int kDsChunk = 8;       // source rows converted per step: two per wave in the horizontal pass
constexpr int kDsMaxTaps = 29;    // coefficients per output position the kernel serves: a ratio of 7
constexpr int kDsMaxLds = 65536;  // dynamic LDS a launch may ask for without a function attribute
constexpr int kDsBits = 22;
constexpr int kDsOutPitch = 3 * kDsTileW;  // bytes of a tile's output row

struct Taps {
  int ksize;
  double scale, support, inv;
};

// One axis of ImagingResample's precompute_coeffs for the bicubic filter: doubles, one rounding per operation.
inline Taps taps_of(int in, int out) {
#pragma clang fp contract(off)
  Taps t;
  t.scale = (double)in / (double)out;
  const double fs = t.scale < 1.0 ? 1.0 : t.scale;
  t.support = 2.0 * fs;
  t.inv = 1.0 / fs;
  t.ksize = (int)__builtin_ceil(t.support) * 2 + 1;
  return t;
}

inline void tap_bounds(const Taps& t, int in, int xx, double& center, int& xmin, int& n) {
#pragma clang fp contract(off)
  center = ((double)xx + 0.5) * t.scale;
  xmin = (int)(center - t.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + t.support + 0.5);
  if (xmax > in) xmax = in;
  n = xmax - xmin;
}

inline double bicubic_weight(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// The source span of every tile of `tile` output positions along one axis, from the bounds alone: the largest
// span (`unit` > 1: with its start moved down to a multiple of `unit` and its length rounded up to one).  A pass
// that does not change the size copies: position xx reads source xx only.
int max_tile_span(int in, int out, int tile, int unit) {
  if (in == out) return ((tile < in ? tile : in) + unit - 1) & ~(unit - 1);
  const Taps t = taps_of(in, out);
  int best = 0;
  for (int x0 = 0; x0 < out; x0 += tile) {
    const int x1 = (x0 + tile < out ? x0 + tile : out) - 1;
    double c;
    int lo, hi, n;
    tap_bounds(t, in, x0, c, lo, n);
    tap_bounds(t, in, x1, c, hi, n);
    lo &= ~(unit - 1);
    const int span = (hi + n - lo + unit - 1) & ~(unit - 1);
    if (span > best) best = span;
  }
  return best;
}

struct DsPlan {
  int ksx, ksy;      // coefficients per output column / row (0: the pass copies)
  int fw, fh;        // LDS capacity: columns of a converted source row, rows of the horizontally filtered tile
  int64_t lds;       // bytes of dynamic LDS
  bool ok;
};

DsPlan ds_plan(int h, int w, int h2, int w2) {
  DsPlan p;
  p.ksx = w2 == w ? 0 : taps_of(w, w2).ksize;
  p.ksy = h2 == h ? 0 : taps_of(h, h2).ksize;
  p.ok = p.ksx <= kDsMaxTaps && p.ksy <= kDsMaxTaps;
  p.fw = p.fh = 0;
  p.lds = 0;
  if (!p.ok) return p;
  p.fw = max_tile_span(w, w2, kDsTileW, 4);
  p.fh = max_tile_span(h, h2, kDsTileH, 1);
  p.lds = 4 * ((int64_t)p.fh * kDsTileW + (int64_t)kDsChunk * p.fw + (int64_t)(p.ksx > 0 ? p.ksx : 1) * kDsTileW) +
          kDsTileH * kDsOutPitch;
  p.ok = p.lds <= kDsMaxLds;
  return p;
}

// The Y, U and V bytes of pixels x0 .. x0 + 3 (x0 % 4 == 0) of row y where every address allows the wide load
// (the caller's `aligned`).  MODE 0: chroma at luma width, 1: halved horizontally (two samples in 16 bits), 2: mono.
template <int MODE>
__device__ __forceinline__ void load_unit_aligned(const uint8_t* __restrict__ frame, int h, int w, const Planes& pl,
                                                  int y, int x0, uint32_t& yd, uint32_t& ud, uint32_t& vd) {
  yd = *reinterpret_cast<const uint32_t*>(frame + (size_t)y * w + x0);
  if (MODE == 2) {
    ud = vd = 0x80808080u;
    return;
  }
  const uint8_t* urow = frame + (size_t)h * w + (size_t)(y >> pl.sy) * pl.cw;
  const size_t csz = (size_t)pl.cw * pl.ch;
  if (MODE == 1) {
    ud = *reinterpret_cast<const uint16_t*>(urow + (x0 >> 1));
    vd = *reinterpret_cast<const uint16_t*>(urow + csz + (x0 >> 1));
  } else {
    ud = *reinterpret_cast<const uint32_t*>(urow + x0);
    vd = *reinterpret_cast<const uint32_t*>(urow + csz + x0);
  }
}

template <int MODE>
__device__ __forceinline__ void convert_unit(uint32_t yd, uint32_t ud, uint32_t vd, uint32_t* __restrict__ dst) {
  uint32_t px[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cs = 8 * (MODE == 1 ? j >> 1 : j);
    px[j] = yuv_pixel((yd >> (8 * j)) & 0xffu, (ud >> cs) & 0xffu, (vd >> cs) & 0xffu);
  }
  *reinterpret_cast<uint4*>(dst) = make_uint4(px[0], px[1], px[2], px[3]);
}

// `rows` <= kDsChunk source rows from y0, `upr` units of 4 pixels from column xa, converted into rgb [rows][pitch]:
// 32 threads per row, each on every 32nd unit of it, the loads of two units issued before either is converted.
template <int MODE>
__device__ __forceinline__ void stage_rows_aligned(const uint8_t* __restrict__ frame, int h, int w, const Planes& pl,
                                                   int y0, int xa, int rows, int upr, uint32_t* __restrict__ rgb,
                                                   int pitch, int tid) {
  constexpr int kPerRow = kBlock / kDsChunk;
  const int ly = tid / kPerRow;
  if (ly >= rows) return;
  uint32_t* row = rgb + ly * pitch;
  for (int q0 = tid & (kPerRow - 1); q0 < upr; q0 += 2 * kPerRow) {
    const bool two = q0 + kPerRow < upr;
    const int q1 = two ? q0 + kPerRow : q0;
    uint32_t ya0, ua0, va0, ya1, ua1, va1;
    load_unit_aligned<MODE>(frame, h, w, pl, y0 + ly, xa + 4 * q0, ya0, ua0, va0);
    load_unit_aligned<MODE>(frame, h, w, pl, y0 + ly, xa + 4 * q1, ya1, ua1, va1);
    convert_unit<MODE>(ya0, ua0, va0, row + 4 * q0);
    if (two) convert_unit<MODE>(ya1, ua1, va1, row + 4 * q1);
  }
}

__device__ __forceinline__ uint32_t ds_round(int acc) {
  const int v = acc >> kDsBits;  // arithmetic shift, as ImagingResample's clip8
  return (uint32_t)min(max(v, 0), 255);
}

// grid (ceil(w2 / kDsTileW), ceil(h2 / kDsTileH), N).  LDS: hres [fhcap][kDsTileW] the horizontally filtered
// pixels of the tile's source rows (r | g << 8 | b << 16), rgb [kDsChunk][fwcap] converted source pixels of the
// rows in flight, kxs [ksx][kDsTileW] the tile's horizontal coefficients (tap-major: lanes read consecutive
// words), obuf [kDsTileH][kDsOutPitch] the tile's output bytes.  ksx / ksy == 0: that pass copies.  The table
// entries are clamped to the staged footprint, so tables that are not vda_resample_tables' cannot make an
// access leave LDS or the source frame.
__global__ __launch_bounds__(kBlock) void yuv_downscale_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int64_t frame_stride, int chroma,
    const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, const int32_t* __restrict__ ky,
    const int32_t* __restrict__ by, int h2, int w2, int ksx, int ksy, int fwcap, int fhcap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ds_lds[];
  uint32_t* hres = ds_lds;
  uint32_t* rgb = hres + (size_t)fhcap * kDsTileW;
  int32_t* kxs = reinterpret_cast<int32_t*>(rgb + (size_t)kDsChunk * fwcap);
  uint8_t* obuf = reinterpret_cast<uint8_t*>(kxs + (size_t)(ksx > 0 ? ksx : 1) * kDsTileW);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the rows a wave takes are scalar
  const int ox0 = blockIdx.x * kDsTileW, oy0 = blockIdx.y * kDsTileH;
  const int nx = min(kDsTileW, w2 - ox0), ny = min(kDsTileH, h2 - oy0);
  const int n = blockIdx.z;

  // the tile's source footprint: bounds are monotone in the output position
  int xa, xe, ya, ye;
  if (ksx > 0) {
    xa = bx[2 * ox0];
    xe = bx[2 * (ox0 + nx - 1)] + bx[2 * (ox0 + nx - 1) + 1];
  } else {
    xa = ox0, xe = ox0 + nx;
  }
  if (ksy > 0) {
    ya = by[2 * oy0];
    ye = by[2 * (oy0 + ny - 1)] + by[2 * (oy0 + ny - 1) + 1];
  } else {
    ya = oy0, ye = oy0 + ny;
  }
  xa = min(max(xa, 0), w - 1) & ~3;
  ya = min(max(ya, 0), h - 1);
  const int upr = min((min(max(xe, xa + 1), w) - xa + 3) >> 2, fwcap >> 2);  // units of 4 pixels per source row
  const int fw = 4 * upr;
  const int fh = min(min(max(ye, ya + 1), h) - ya, fhcap);

  // this lane's output column: first staged source column, taps
  const int oxl = min(lane, nx - 1);
  int xs = 0, nt = 1;
  if (ksx > 0) {
    xs = bx[2 * (ox0 + oxl)] - xa;
    nt = bx[2 * (ox0 + oxl) + 1];
    for (int i = tid; i < ksx * kDsTileW; i += kBlock) {
      const int t = i / kDsTileW, c = i - t * kDsTileW;
      kxs[i] = c < nx ? kx[(size_t)(ox0 + c) * ksx + t] : 0;
    }
  } else {
    xs = ox0 + oxl - xa;
  }
  xs = min(max(xs, 0), fw - 1);
  nt = min(min(max(nt, 0), ksx > 0 ? ksx : 1), fw - xs);

  const Planes pl = planes_of(h, w, chroma);
  const uint8_t* frame = src + (size_t)n * frame_stride;
  // w % 4 == 0 and dword-aligned frames: every unit is whole and every plane row dword-aligned (chroma rows of a
  // subsampled plane 16-bit-aligned), so the units load without branches and two are in flight per thread
  const bool aligned = (w & 3) == 0 && (((uintptr_t)src | (uintptr_t)frame_stride) & 3) == 0;
  for (int r0 = 0; r0 < fh; r0 += kDsChunk) {
    const int rows = min(kDsChunk, fh - r0);
    __syncthreads();  // the previous chunk's rows have been filtered (first pass: nothing to wait for but kxs)
    if (aligned) {
      if (chroma == VDA_YUV_MONO) stage_rows_aligned<2>(frame, h, w, pl, ya + r0, xa, rows, upr, rgb, fwcap, tid);
      else if (pl.sx) stage_rows_aligned<1>(frame, h, w, pl, ya + r0, xa, rows, upr, rgb, fwcap, tid);
      else stage_rows_aligned<0>(frame, h, w, pl, ya + r0, xa, rows, upr, rgb, fwcap, tid);
    } else {
      for (int u = tid; u < rows * upr; u += kBlock) {
        const int ly = u / upr, q = u - ly * upr;
        uint32_t px[4];
        convert4_any(chroma, frame, h, w, pl, ya + r0 + ly, xa + 4 * q, px);
        *reinterpret_cast<uint4*>(&rgb[ly * fwcap + 4 * q]) = make_uint4(px[0], px[1], px[2], px[3]);
      }
    }
    __syncthreads();
    // horizontal pass: a wave takes two of the chunk's rows, a lane one output column of both
    const int l0 = 2 * wave, l1 = l0 + 1;
    if (l0 < rows) {
      const uint32_t* p0 = rgb + l0 * fwcap + xs;
      const uint32_t* p1 = l1 < rows ? p0 + fwcap : p0;
      int a0[3], a1[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) a0[c] = a1[c] = 1 << (kDsBits - 1);
      for (int t = 0; t < nt; ++t) {
        const int cf = ksx > 0 ? kxs[t * kDsTileW + lane] : (1 << kDsBits);
        const uint32_t u0 = p0[t], u1 = p1[t];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a0[c] += __mul24((int)((u0 >> (8 * c)) & 0xffu), cf);
          a1[c] += __mul24((int)((u1 >> (8 * c)) & 0xffu), cf);
        }
      }
      hres[(r0 + l0) * kDsTileW + lane] = ds_round(a0[0]) | (ds_round(a0[1]) << 8) | (ds_round(a0[2]) << 16);
      if (l1 < rows)
        hres[(r0 + l1) * kDsTileW + lane] = ds_round(a1[0]) | (ds_round(a1[1]) << 8) | (ds_round(a1[2]) << 16);
    }
  }
  __syncthreads();

  // vertical pass: a wave takes output rows wave, wave + kDsWaves, ...; the row's taps are wave-uniform
  for (int ly = wave; ly < ny; ly += kDsWaves) {
    const int oy = oy0 + ly;
    int ys, mt;
    if (ksy > 0) {
      ys = __builtin_amdgcn_readfirstlane(by[2 * oy]) - ya;
      mt = __builtin_amdgcn_readfirstlane(by[2 * oy + 1]);
    } else {
      ys = oy - ya, mt = 1;
    }
    ys = min(max(ys, 0), fh - 1);
    mt = min(min(max(mt, 0), ksy > 0 ? ksy : 1), fh - ys);
    const int32_t* krow = ky + (size_t)oy * ksy;
    const uint32_t* p = hres + ys * kDsTileW + lane;
    int acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = 1 << (kDsBits - 1);
    for (int t = 0; t < mt; ++t) {
      const int cf = ksy > 0 ? __builtin_amdgcn_readfirstlane(krow[t]) : (1 << kDsBits);
      const uint32_t u = p[t * kDsTileW];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += __mul24((int)((u >> (8 * c)) & 0xffu), cf);
    }
    uint8_t* o = obuf + ly * kDsOutPitch + 3 * lane;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)ds_round(acc[c]);
  }
  __syncthreads();

  // store: 16 threads per output row; the run of 3 * nx bytes goes out as a bytewise head up to the first
  // dword-aligned address, dwords, and a bytewise tail
  const int ly = tid >> 4, l16 = tid & 15;
  if (ly < ny) {
    uint8_t* g = dst + (((size_t)n * h2 + oy0 + ly) * w2 + ox0) * 3;
    const uint8_t* s = obuf + ly * kDsOutPitch;
    const int len = 3 * nx;
    const int head = min((int)((4 - ((uintptr_t)g & 3)) & 3), len);
    const int nd = (len - head) >> 2;
    const int tail0 = head + 4 * nd;
    if (l16 < head) g[l16] = s[l16];
    for (int i = l16; i < nd; i += 16) {
      const int off = head + 4 * i;
      const uint32_t v = (uint32_t)s[off] | ((uint32_t)s[off + 1] << 8) | ((uint32_t)s[off + 2] << 16) |
                         ((uint32_t)s[off + 3] << 24);
      *reinterpret_cast<uint32_t*>(g + off) = v;
    }
    if (l16 < len - tail0) g[tail0 + l16] = s[tail0 + l16];
  }
}

}  // namespace

extern "C" int32_t vda_resample_taps(int32_t in, int32_t out) {
  if (in < 1 || out < 1) return 0;
  return taps_of(in, out).ksize;
}

extern "C" int vda_resample_tables(int32_t in, int32_t out, int32_t* k, int32_t* bounds) {
#pragma clang fp contract(off)
  VDA_CHECK_ARG(k && bounds, "null pointer");
  VDA_CHECK_ARG(in > 0 && out > 0, "empty axis");
  const Taps t = taps_of(in, out);
  for (int xx = 0; xx < out; ++xx) {
    double center;
    int xmin, n;
    tap_bounds(t, in, xx, center, xmin, n);
    // the weights are computed twice, to sum them in order and then to normalise them: no buffer
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += bicubic_weight(((double)(x + xmin) - center + 0.5) * t.inv);
    int32_t* row = k + (size_t)xx * t.ksize;
    for (int x = 0; x < t.ksize; ++x) {
      if (x >= n) {
        row[x] = 0;
        continue;
      }
      double v = bicubic_weight(((double)(x + xmin) - center + 0.5) * t.inv);
      if (ww != 0.0) v /= ww;
      row[x] = (int32_t)(v * (double)(1 << kDsBits) + (v < 0.0 ? -0.5 : 0.5));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return 0;
}

extern "C" int vda_yuv_downscale_ok(int32_t h, int32_t w, int32_t h2, int32_t w2) {
  if (h < 1 || w < 1 || h2 < 1 || w2 < 1) return 0;
  return ds_plan(h, w, h2, w2).ok ? 1 : 0;
}

extern "C" int64_t vda_yuv_downscale_workspace(int32_t N, int32_t h, int32_t w, int32_t h2, int32_t w2) {
  (void)N, (void)h, (void)w, (void)h2, (void)w2;
  return 0;  // one route: the tile kernel, which keeps its intermediates in LDS
}

extern "C" int vda_yuv_downscale(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride,
                                 int32_t chroma, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                                 const int32_t* by, uint8_t* out, int32_t h2, int32_t w2, void* ws, int64_t ws_bytes,
                                 void* stream) {
  (void)ws, (void)ws_bytes;
  VDA_CHECK_ARG(src && out, "null pointer");
  VDA_CHECK_ARG(N > 0 && h > 0 && w > 0 && h2 > 0 && w2 > 0, "empty frame geometry");
  VDA_CHECK_ARG(chroma_ok(chroma), "unknown chroma code (VDA_YUV_420, VDA_YUV_422, VDA_YUV_444 or VDA_YUV_MONO)");
  VDA_CHECK_ARG(frame_stride >= payload_bytes(h, w, chroma), "frame_stride below the frame's payload size");
  VDA_CHECK_ARG(h2 <= kMaxGridYZ && N <= kMaxGridYZ, "output height / frame count exceed the launch grid");
  const DsPlan p = ds_plan(h, w, h2, w2);
  VDA_CHECK_ARG(p.ok, "downscale ratio beyond the kernel's tap capacity (vda_yuv_downscale_ok)");
  VDA_CHECK_ARG((p.ksx == 0 || (kx && bx)) && (p.ksy == 0 || (ky && by)), "null coefficient table for a resampled axis");
  hipLaunchKernelGGL(yuv_downscale_kernel, dim3((w2 + kDsTileW - 1) / kDsTileW, (h2 + kDsTileH - 1) / kDsTileH, N),
                     dim3(kBlock), (size_t)p.lds, (hipStream_t)stream, src, out, h, w, frame_stride, chroma, kx, bx, ky,
                     by, h2, w2, p.ksx, p.ksy, p.fw, p.fh);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_yuv_to_rgb(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride,
                              int32_t chroma, uint8_t* out, void* stream) {
  VDA_CHECK_ARG(src && out, "null pointer");
  VDA_CHECK_ARG(N > 0 && h > 0 && w > 0, "empty frame geometry");
  VDA_CHECK_ARG(chroma_ok(chroma), "unknown chroma code (VDA_YUV_420, VDA_YUV_422, VDA_YUV_444 or VDA_YUV_MONO)");
  VDA_CHECK_ARG(frame_stride >= payload_bytes(h, w, chroma), "frame_stride below the frame's payload size");
  VDA_CHECK_ARG(h <= kMaxGridYZ && N <= kMaxGridYZ, "frame height / frame count exceed the launch grid");
  const int units = (w + 3) / 4;
  hipLaunchKernelGGL(yuv_to_rgb_kernel, dim3((units + kBlock - 1) / kBlock, h, N), dim3(kBlock), 0, (hipStream_t)stream,
                     src, out, h, w, frame_stride, chroma);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vda_preprocess_yuv_workspace(int32_t N, int32_t h, int32_t w, int32_t H, int32_t W) {
  if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return 0;
  if (footprint_bound(h, w, H, W) <= kCapPx) return 0;
  return ((int64_t)N * h * w * 3 + 255) / 256 * 256;
}

extern "C" int vda_preprocess_yuv(const uint8_t* src, int32_t N, int32_t h, int32_t w, int64_t frame_stride,
                                  int32_t chroma, float* out, int32_t H, int32_t W, const float* mean,
                                  const float* stdv, void* ws, int64_t ws_bytes, void* stream) {
  VDA_CHECK_ARG(src && out && mean && stdv, "null pointer");
  VDA_CHECK_ARG(N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "empty frame geometry");
  VDA_CHECK_ARG(chroma_ok(chroma), "unknown chroma code (VDA_YUV_420, VDA_YUV_422, VDA_YUV_444 or VDA_YUV_MONO)");
  VDA_CHECK_ARG(frame_stride >= payload_bytes(h, w, chroma), "frame_stride below the frame's payload size");
  VDA_CHECK_ARG(H <= kMaxGridYZ && N <= kMaxGridYZ, "output height / frame count exceed the launch grid");
  NormArgs na;
  for (int c = 0; c < 3; ++c) {
    VDA_CHECK_ARG(stdv[c] != 0.f, "std must be non-zero");
    na.mean[c] = mean[c];
    na.std_[c] = stdv[c];
  }
  const int64_t need = vda_preprocess_yuv_workspace(N, h, w, H, W);
  if (need > 0) {  // composition route: the RGB frames in the workspace, then the RGB kernel
    VDA_CHECK_ARG(ws && ws_bytes >= need, "workspace smaller than vda_preprocess_yuv_workspace(N, h, w, H, W)");
    const int rc = vda_yuv_to_rgb(src, N, h, w, frame_stride, chroma, (uint8_t*)ws, stream);
    if (rc != 0) return rc;
    return vda_preprocess_frames(ws, out, N, h, w, H, W, mean, stdv, stream);
  }
  hipLaunchKernelGGL(preprocess_yuv_kernel, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, N), dim3(kBlock),
                     0, (hipStream_t)stream, src, out, h, w, frame_stride, chroma, H, W, na);
  VDA_LAUNCH_CHECK();
  return 0;
}
