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

}  // namespace

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
