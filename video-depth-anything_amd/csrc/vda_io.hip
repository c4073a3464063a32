// Frame preprocessing and depth post-resize: the data formats either side of the clip forward.
//
// preprocess: uint8 RGB frames [N, h, w, 3] (HWC, as decoded video frames arrive) -> the network
// input [N, 3, H, W] float: x / 255, bicubic resize (a = -0.75, half-pixel centres, clamped
// borders, no antialias: cv2.INTER_CUBIC == torch bicubic align_corners=False), then
// (x - mean) / std.  Replaces util/transform.py:5-157 (Resize + NormalizeImage + PrepareForNet)
// as applied per frame in video_depth.py:336-361 / :140-146 / :209.
//
// depth_resize: depth [N, H, W] float -> [N, ho, wo] float, bilinear align_corners=True
// (video_depth.py:372, :300).
//
// Both are HBM/latency-bound elementwise gathers: one thread per output pixel, consecutive
// threads on consecutive output columns so every store is a coalesced row segment; the 4x4 (or
// 2x2) source window of neighbouring threads overlaps and is served from L1/L2.
#include "vda_preprocess.h"
#include "../../include/vda.h"

namespace {

using vda_pre::NormArgs;

// Source pixel (y, x) of an interleaved RGB frame.
struct RgbFetch {
  const uint8_t* frame;
  int w;
  __device__ __forceinline__ vda_pre::Px operator()(int y, int x) const {
    const uint8_t* p = frame + ((size_t)y * w + x) * 3;
    return {{vda_pre::unit_scale(p[0]), vda_pre::unit_scale(p[1]), vda_pre::unit_scale(p[2])}};
  }
};

// The per-pixel arithmetic is vda_pre::preprocess_pixel, shared with vda_preprocess_yuv (vda_decode.hip).
__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                         int h, int w, int H, int W, NormArgs na) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  const int oy = blockIdx.y;
  const int n = blockIdx.z;
  if (ox >= W) return;
  const RgbFetch fetch{src + (size_t)n * h * w * 3, w};
  const size_t plane = (size_t)H * W;
  vda_pre::preprocess_pixel(fetch, h, w, H, W, oy, ox, na, dst + (size_t)n * 3 * plane + (size_t)oy * W + ox, plane);
}

__global__ __launch_bounds__(256) void depth_resize_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int H, int W, int ho, int wo) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  const int oy = blockIdx.y;
  const int n = blockIdx.z;
  if (ox >= wo) return;
  dst[((size_t)n * ho + oy) * wo + ox] = depth_bilinear_ac(src + (size_t)n * H * W, H, W, ho, wo, oy, ox);
}

}  // namespace

extern "C" int vda_preprocess_frames(const void* frames, float* out, int32_t N, int32_t h, int32_t w, int32_t H,
                                     int32_t W, const float* mean, const float* stdv, void* stream) {
  VDA_CHECK_ARG(frames && out && mean && stdv, "null pointer");
  VDA_CHECK_ARG(N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "empty frame geometry");
  VDA_CHECK_ARG(H <= 65535 && N <= 65535, "output height / frame count exceed the launch grid");
  NormArgs na;
  for (int c = 0; c < 3; ++c) {
    VDA_CHECK_ARG(stdv[c] != 0.f, "std must be non-zero");
    na.mean[c] = mean[c];
    na.std_[c] = stdv[c];
  }
  hipLaunchKernelGGL(preprocess_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)frames, out, h, w, H, W, na);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_depth_resize(const float* depth, float* out, int32_t N, int32_t H, int32_t W, int32_t ho,
                                int32_t wo, void* stream) {
  VDA_CHECK_ARG(depth && out, "null pointer");
  VDA_CHECK_ARG(N > 0 && H > 0 && W > 0 && ho > 0 && wo > 0, "empty depth geometry");
  VDA_CHECK_ARG(ho <= 65535 && N <= 65535, "output height / frame count exceed the launch grid");
  hipLaunchKernelGGL(depth_resize_kernel, dim3((wo + 255) / 256, ho, N), dim3(256), 0, (hipStream_t)stream, depth, out,
                     H, W, ho, wo);
  VDA_LAUNCH_CHECK();
  return 0;
}
