// One output pixel of the frame preprocessing (x / 255, bicubic resize, normalise): the single definition
// behind vda_preprocess_frames (source pixels read from interleaved RGB in global memory, vda_io.hip) and
// vda_preprocess_yuv (source pixels converted from planar YUV once and read from LDS, vda_decode.hip).  Both
// kernels instantiate preprocess_pixel, so the coordinates, the weights and the accumulation order are the
// same expressions in both and their outputs agree bit for bit.
#pragma once
#include "vda_common.h"

namespace vda_pre {

constexpr float kCubicA = -0.75f;

// torch upsample_bicubic2d / cv2 INTER_CUBIC kernel weights for fractional offset t
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = kCubicA;
  const float x0 = t + 1.f;   // |x| in (1, 2)
  const float x1 = t;         // |x| in [0, 1]
  const float x2 = 1.f - t;   // |x| in [0, 1]
  const float x3 = 2.f - t;   // |x| in (1, 2)
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

struct NormArgs {
  float mean[3];
  float std_[3];
};

// half-pixel source coordinate of output index o, not clamped (cubic): torch
// area_pixel_compute_source_index(cubic=true)
__device__ __forceinline__ float src_coord(int in, int out, int o) {
  return (float)in / (float)out * ((float)o + 0.5f) - 0.5f;
}

// A source pixel as the resize takes it: its three channels / 255 (unit_scale, one IEEE division each; where a
// kernel evaluates it does not change its bits, so a kernel that keeps source pixels may do it once per pixel).
struct Px {
  float c[3];
};
__device__ __forceinline__ float unit_scale(uint32_t byte) { return (float)byte / 255.f; }

// Output pixel (oy, ox) of a frame [h, w] resized to [H, W]: out[c * plane] for c = 0..2.  fetch(y, x) returns
// source pixel (y, x), both already clamped to the frame, as a Px.
template <class Fetch>
__device__ __forceinline__ void preprocess_pixel(const Fetch& fetch, int h, int w, int H, int W, int oy, int ox,
                                                 const NormArgs& na, float* __restrict__ out, size_t plane) {
  const float sy = src_coord(h, H, oy);
  const float sx = src_coord(w, W, ox);
  const float fy = floorf(sy), fx = floorf(sx);
  const int iy = (int)fy, ix = (int)fx;
  float wy[4], wx[4];
  cubic_weights(sy - fy, wy);
  cubic_weights(sx - fx, wx);
  int cols[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cols[k] = min(max(ix - 1 + k, 0), w - 1);
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = min(max(iy - 1 + r, 0), h - 1);
    float rv[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Px p = fetch(row, cols[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) rv[c] += p.c[c] * wx[k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += rv[c] * wy[r];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c * plane] = (acc[c] - na.mean[c]) / na.std_[c];
}

}  // namespace vda_pre
