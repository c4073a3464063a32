// Looked-up pixels to bytes: what the kernels that turn fp32 maps into the bytes of an image file share
// (vda_vis.hip colours one depth video, vda_compare.hip composes a canvas of tiles).  The colour index
// rule, the 256-row table in LDS and the three ways a frame of packed pixels r | g << 8 | b << 16 goes
// out (planes, interleaved rows, 4:2:0 strips) are defined here and nowhere else; where the pixels come
// from is the kernel's own (a functor).
// Stores are dwords: frames and planes start at byte offsets that are not multiples of 4 in general, so
// every plane is a streaming pass (vda_stream.h, split by the dword rule on the destination) with a
// bytewise head and tail of at most 3 pixels around the body.
#pragma once
#include "vda_stream.h"

typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));

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

// NPL planes of one frame of S pixels that share their alignment: plane c at dst + c * pstride holds byte c
// of every pixel.  get4(o, v) gives the packed pixels o .. o + 3, get1(e) the pixel e.  Head and tail pixels
// (at most 3 each) are stored bytewise by block 0, the body as one dword per plane and group of 4 pixels.
template <int NPL, class Get4, class Get1>
__device__ __forceinline__ void planes_pass(int64_t S, uint8_t* __restrict__ dst, int64_t pstride, Get4&& get4,
                                            Get1&& get1) {
  const StreamSplit sp = stream_split_u8(dst, 1, S);
  stream_walk(
      S, sp.head, sp.nvec,
      [&](int64_t o) {
        uint32_t v[4];
        get4(o, v);
#pragma unroll
        for (int c = 0; c < NPL; ++c) {
          const uint32_t w = ((v[0] >> (8 * c)) & 0xffu) | (((v[1] >> (8 * c)) & 0xffu) << 8) |
                             (((v[2] >> (8 * c)) & 0xffu) << 16) | (((v[3] >> (8 * c)) & 0xffu) << 24);
          *reinterpret_cast<uint32_t*>(dst + c * pstride + o) = w;
        }
      },
      [&](int64_t e) {
        const uint32_t v = get1(e);
#pragma unroll
        for (int c = 0; c < NPL; ++c) dst[c * pstride + e] = (uint8_t)(v >> (8 * c));
      });
}

// Interleaved rows: pixel p of the frame at dst + 3 p.  A group of 4 pixels is 12 bytes = three dwords.
// The top byte of a packed pixel must be 0.
template <class Get4, class Get1>
__device__ __forceinline__ void hwc_pass(int64_t S, uint8_t* __restrict__ dst, Get4&& get4, Get1&& get1) {
  const StreamSplit sp = stream_split_u8(dst, 3, S);
  stream_walk(
      S, sp.head, sp.nvec,
      [&](int64_t o) {
        uint32_t v[4];
        get4(o, v);
        u32x3a4 w;
        w[0] = v[0] | (v[1] << 24);
        w[1] = (v[1] >> 8) | (v[2] << 16);
        w[2] = (v[2] >> 16) | (v[3] << 8);
        *reinterpret_cast<u32x3a4*>(dst + 3 * o) = w;
      },
      [&](int64_t e) {
        const uint32_t v = get1(e);
        dst[3 * e] = (uint8_t)v;
        dst[3 * e + 1] = (uint8_t)(v >> 8);
        dst[3 * e + 2] = (uint8_t)(v >> 16);
      });
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

// One 4:2:0 strip of 8 x 2 packed pixels v (columns and rows past the edge already repeated): nv luma bytes
// (byte 0) to yrow and, with `two`, to yrow + W; nc bytes of each chroma plane (bytes 1 and 2), every one
// (a + b + c + d + 2) >> 2 over its 2x2 block, to up and vp.
__device__ __forceinline__ void store_strip_420(const uint32_t (&v)[2][8], uint8_t* yrow, int64_t W, bool two, int nv,
                                                uint8_t* up, uint8_t* vp, int nc) {
  uint32_t yw[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      yw[r][h] = (v[r][4 * h] & 0xffu) | ((v[r][4 * h + 1] & 0xffu) << 8) | ((v[r][4 * h + 2] & 0xffu) << 16) |
                 ((v[r][4 * h + 3] & 0xffu) << 24);
  }
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
  store_strip(up, uw, nc);
  store_strip(vp, vw, nc);
}
