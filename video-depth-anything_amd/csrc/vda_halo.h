// What the halo-tiled conv kernels share (vda_depth.hip, vda_dconv.hip, vda_hconv.hip, vda_strip.hip) and
// the resize kernel with them (vda_misc.hip): the LDS-DMA and wait primitives, the geometry of a tile and
// of the source window its fused-resize patch needs, and the separable blend that builds that patch.  A
// kernel keeps its own LDS layout, thread-to-item mapping and pipeline; what is defined here is defined
// nowhere else.  The align_corners coordinate helpers (ac_scale, ac_coord, ac_weight) are in vda_common.h,
// because the fp32 resizes there and in vda_f32.hip form the same scale.
#pragma once
#include "vda_common.h"

// ---- primitives ------------------------------------------------------------------------------
// 16 B per lane HBM -> LDS without a VGPR (global_load_lds_dwordx4): lane l lands at lds_base + 16 l
__device__ __forceinline__ void glds16(const void* src, h16* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (VDA_LDS void*)lds_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// lgkmcnt(0) as the builtin (vmcnt / expcnt untouched): the compiler then knows the LDS reads before it
// are complete and adds no wait of its own for them later; it also retires asm LDS stores, which the
// compiler's counts do not see
__device__ __forceinline__ void lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// ---- tiles -----------------------------------------------------------------------------------
// A launch over T x T output tiles of BT maps [H, W], persistent blocks taking tiles t = block + i * grid.
struct HaloGrid {
  int tiles_x, tiles_y, ntiles, grid;
};
// false: more than `limit` tiles (the caller's error).  grid = min(ntiles, blocks_per_cu * CUs).
inline bool halo_tile_grid(int BT, int H, int W, int T, int blocks_per_cu, long limit, HaloGrid& g) {
  g.tiles_x = (W + T - 1) / T;
  g.tiles_y = (H + T - 1) / T;
  const long nt = (long)BT * g.tiles_x * g.tiles_y;
  if (nt > limit) return false;
  g.ntiles = (int)nt;
  const int cap = blocks_per_cu * vda_cu_count();
  g.grid = g.ntiles < cap ? g.ntiles : cap;
  return true;
}
// tile t in the plain order (x fastest, then y, then the map) -> map bt, first output row / column
__device__ __forceinline__ void halo_tile_of(int t, int tiles_x, int tiles_y, int T, int& bt, int& y0, int& x0) {
  const int tx = t % tiles_x;
  const int r = t / tiles_x;
  const int ty = r % tiles_y;
  bt = r / tiles_y;
  y0 = ty * T;
  x0 = tx * T;
}

// ---- fused resize: the source window of a patch ------------------------------------------------
// The (T + 2)^2 patch of the tile at (y0, x0) of the resized [H, W] map reads source rows sy_lo ..
// sy_lo + SR - 1 and columns sx_lo .. sx_lo + SC - 1 of the [Hs, Ws] map (usy / usx = ac_scale).
__device__ __forceinline__ void halo_src_region(float usy, float usx, int y0, int x0, int T, int H, int W, int Hs,
                                                int Ws, int& sy_lo, int& sx_lo, int& SR, int& SC) {
  sy_lo = (int)(usy * (float)max(y0 - 1, 0));
  sx_lo = (int)(usx * (float)max(x0 - 1, 0));
  SR = min((int)(usy * (float)min(y0 + T, H - 1)) + 1, Hs - 1) - sy_lo + 1;
  SC = min((int)(usx * (float)min(x0 + T, W - 1)) + 1, Ws - 1) - sx_lo + 1;
}
// The kernels stage that window in an LDS slot of HALO_SRC_PIXELS pixels; a 16 x 16 tile's window is at
// most floor(17 * scale) + 3 pixels a side.  The one test behind every fused route and workspace query.
constexpr int HALO_SRC_PIXELS = 192;
inline bool halo_fused_fits(int Hs, int Ws, int H, int W) {
  const float sy = ac_scale(Hs, H), sx = ac_scale(Ws, W);
  return ((int)(17.f * sy) + 3) * ((int)(17.f * sx) + 3) <= HALO_SRC_PIXELS;
}

// ---- fused resize: the separable blend ---------------------------------------------------------
// SEG consecutive patch rows pr0 .. pr0 + SEG - 1 of patch column `col` (map column x0 - 1 + col), one
// 16-B channel chunk.  The blend is o = fma(wy, bot, uy * top) with top / bot the horizontal blends
// fma(wx, B, ux * A) of source rows sy0 / sy1 at the column; a source row's horizontal blend does not
// depend on the output row that uses it, so it is formed once per (column, source row) and carried down
// the segment: per pixel the ops of bilerp8_mix, bit-identical to bilerp8 (the resize kernel's blend), in
// about half its VALU.  src(row, column) reads the chunk of a staged source pixel, row and column counted
// from the staged window's first (sy_lo, sx_lo of halo_src_region); put(patch row, value) stores a patch
// pixel (zero outside the map).  Both are the caller's, as are the item mapping and the lgkmcnt wait its
// store form needs afterwards.
template <int SEG, class Src, class Put>
__device__ __forceinline__ void halo_blend_column(float usy, float usx, int y0, int x0, int col, int pr0, int H, int W,
                                                  int Hs, int Ws, int sy_lo, int sx_lo, Src&& src, Put&& put) {
  const int pxg = x0 - 1 + col;
  const bool okx = (unsigned)pxg < (unsigned)W;
  int sx0, sx1;
  float wx;
  ac_coord(min(max(pxg, 0), W - 1), Ws, usx, sx0, sx1, wx);
  const float ux = 1.f - wx;
  const int c0 = sx0 - sx_lo, c1 = sx1 - sx_lo;
  auto hrow = [&](int sy, float (&t)[8]) {
    const uint4 a = src(sy - sy_lo, c0), b = src(sy - sy_lo, c1);
    const unsigned A[4] = {a.x, a.y, a.z, a.w}, B[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[2 * j] = fma_mix_lo(wx, B[j], fma_mix_lo(ux, A[j], -0.f));
      t[2 * j + 1] = fma_mix_hi(wx, B[j], fma_mix_hi(ux, A[j], -0.f));
    }
  };
  float top[8], bot[8];
  int s0 = -1, s1 = -1;
#pragma unroll
  for (int k = 0; k < SEG; ++k) {
    const int pr = pr0 + k;
    const int pyg = y0 - 1 + pr;
    int sy0, sy1;
    float wy;
    ac_coord(min(max(pyg, 0), H - 1), Hs, usy, sy0, sy1, wy);
    const float uy = 1.f - wy;
    if (sy0 != s0) {  // scale <= 1: the source rows advance by at most one per output row
      if (sy0 == s1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) top[e] = bot[e];
      } else {
        hrow(sy0, top);
      }
      hrow(sy1, bot);
      s0 = sy0;
      s1 = sy1;
    }
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float ol = fma_f32(wy, bot[2 * j], mul_f32(uy, top[2 * j]));
      const float oh = fma_f32(wy, bot[2 * j + 1], mul_f32(uy, top[2 * j + 1]));
      typedef float f2v __attribute__((ext_vector_type(2)));
      o[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{ol, oh}, h2));
    }
    const bool ok = okx && (unsigned)pyg < (unsigned)H;
    put(pr, ok ? make_uint4(o[0], o[1], o[2], o[3]) : make_uint4(0u, 0u, 0u, 0u));
  }
}
