// Sub-pixel conv: ConvTranspose2d(k = s) followed by a zero-padded 3x3 conv, composed into one linear map of the
// low-resolution input (include/vda.h vda_subpixel_conv).  Output phase (a, b) of source pixel (i, j) sees a
// 1x1, 1x2, 2x1 or 2x2 window of source pixels, so the work is a handful of dense GEMMs on ONE "corner" matrix:
// row (bt, ci, cj), ci in [0, h], cj in [0, w], holds the four source pixels around corner (ci, cj) in the block
// order [p(ci-1, cj-1) | p(ci, cj-1) | p(ci, cj) | p(ci-1, cj)] (zeros outside the frame: a window never reads
// the neighbouring frame).  Every window shape is then a contiguous K slice of that row:
//   2x2 = all four blocks, 1x2 = blocks 1..2, 2x1 = blocks 2..3, 1x1 = block 2,
// and phase (a, b) of source pixel (i, j) reads corner (i + (a == s - 1), j + (b == s - 1)).  Each group of four
// phases with one window shape is one launch of the phased 256x256 GEMM (vda_gemm_phased.h, SUBP epilogue), which
// adds the 9-class bias and writes each corner row as the 512-B channel run of its output pixel.
#include "vda_internal.h"
#include <algorithm>

namespace {

// One 16-B chunk per thread; block y walks the corner rows.
__global__ __launch_bounds__(256) void corner_gather_kernel(const h16* __restrict__ x, h16* __restrict__ a, int M, int H,
                                                            int W, int Cin) {
  const int cpt = Cin >> 3;  // 16-B chunks per block
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 4 * cpt) return;
  const int blk = c / cpt, cc = c - blk * cpt;
  const int dy = (blk == 0 || blk == 3) ? -1 : 0, dx = blk < 2 ? -1 : 0;
  const int hc = H + 1, wc = W + 1;
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    const int bt = m / (hc * wc), r = m - bt * (hc * wc), ci = r / wc, cj = r - ci * wc;
    const int iy = ci + dy, ix = cj + dx;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
      v = ldg16(x + (((long)bt * H + iy) * W + ix) * Cin + cc * 8);
    stg16(a + ((long)m * 4 * cpt + c) * 8, v);
  }
}

struct Group {
  int koff, kblocks;  // K slice of the corner row, in blocks of Cin
  int phases;         // four (a << 2 | b) nibbles, N tile order
};
constexpr int ph4(int a0, int b0, int a1, int b1, int a2, int b2, int a3, int b3) {
  return (a0 << 2 | b0) | (a1 << 2 | b1) << 4 | (a2 << 2 | b2) << 8 | (a3 << 2 | b3) << 12;
}
// the order of the weight groups in `w` (include/vda.h)
const Group G2[] = {{0, 4, ph4(0, 0, 0, 1, 1, 0, 1, 1)}};
const Group G4[] = {{0, 4, ph4(0, 0, 0, 3, 3, 0, 3, 3)},
                    {1, 2, ph4(1, 0, 1, 3, 2, 0, 2, 3)},
                    {2, 2, ph4(0, 1, 0, 2, 3, 1, 3, 2)},
                    {2, 1, ph4(1, 1, 1, 2, 2, 1, 2, 2)}};

int check(int BT, int h, int w, int Cin, int Cout, int s) {
  VDA_CHECK_ARG(BT > 0 && h > 0 && w > 0 && Cin > 0, "sub-pixel conv: empty map");
  VDA_CHECK_ARG(s == 2 || s == 4, "sub-pixel conv: s must be 2 or 4");
  VDA_CHECK_ARG(Cout == 256 && Cin % 64 == 0, "sub-pixel conv: Cout == 256 and Cin % 64 == 0");
  const long M = (long)BT * (h + 1) * (w + 1);
  VDA_CHECK_ARG(M * 4 * Cin * 2 < (1L << 31) && (long)BT * h * s * w * s * Cout * 2 < (1L << 31) &&
                    (long)BT * h * w * Cin * 2 < (1L << 31),
                "sub-pixel conv: the corner matrix, the input and the output must each stay below 2 GiB");
  return 0;
}

}  // namespace

extern "C" int vda_subpixel_conv_check(int32_t BT, int32_t h, int32_t w, int32_t Cin, int32_t Cout, int32_t s) {
  return check(BT, h, w, Cin, Cout, s);
}

extern "C" int64_t vda_subpixel_conv_workspace(int32_t BT, int32_t h, int32_t w, int32_t Cin, int32_t s) {
  if (check(BT, h, w, Cin, 256, s)) return 0;
  return (int64_t)BT * (h + 1) * (w + 1) * 4 * Cin * 2;
}

extern "C" int vda_subpixel_conv(const void* x, const void* w, const float* bias9, void* y, int32_t BT, int32_t h,
                                 int32_t w_, int32_t Cin, int32_t Cout, int32_t s, void* ws, int64_t ws_bytes,
                                 void* stream) {
  VDA_CHECK_ARG(x && w && bias9 && y && ws, "null pointer");
  int rc = check(BT, h, w_, Cin, Cout, s);
  if (rc) return rc;
  VDA_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)ws % 16 == 0 &&
                    (uintptr_t)bias9 % 16 == 0,
                "sub-pixel conv: x, w, bias9, y and ws must be 16-byte aligned");
  const int M = BT * (h + 1) * (w_ + 1);
  VDA_CHECK_ARG(ws_bytes >= (int64_t)M * 4 * Cin * 2, "sub-pixel conv: workspace too small (vda_subpixel_conv_workspace)");
  hipStream_t st = (hipStream_t)stream;
  const int cpr = 4 * (Cin / 8);
  hipLaunchKernelGGL(corner_gather_kernel, dim3((unsigned)((cpr + 255) / 256), (unsigned)std::min(M, 65535)), dim3(256), 0,
                     st, (const h16*)x, (h16*)ws, M, h, w_, Cin);
  VDA_LAUNCH_CHECK();
  const Group* g = s == 2 ? G2 : G4;
  const int ng = s == 2 ? 1 : 4;
  const h16* wg = (const h16*)w;
  for (int i = 0; i < ng; ++i) {
    GemmParams p{};
    p.x = (const h16*)ws + (long)g[i].koff * Cin;
    p.ldx = 4L * Cin;
    p.w = wg;
    p.y = (h16*)y;
    p.ldy = Cout;
    p.M = M; p.N = 4 * Cout; p.K = g[i].kblocks * Cin;
    p.H = h; p.W = w_; p.stride = s;
    p.epi = vda_default_epi();
    p.sp_bt = BT; p.sp_phases = g[i].phases; p.sp_bias = bias9;
    rc = vda_launch_subpixel_gemm(p, st);
    if (rc) return rc;
    wg += (long)p.N * p.K;
  }
  return 0;
}
