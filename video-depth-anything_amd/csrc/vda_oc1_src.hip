// output_conv1 on the x2 bilinear (align_corners=True) resize of x, with the channel mixing done at the
// SOURCE resolution: conv and resize are both linear, so
//
//   out(p) = b(class of p) + sum_t [p + d_t inside the 2h x 2w map] * bilerp(z_t, p + d_t),   z_t = W_t x  at h x w
//
// (t over the 9 taps, d_t the tap's offset, the bracket the conv's zero padding on the output grid).  The
// halo conv with the fused resize (vda_oc1.hip) interpolates each 18 x 18 patch and multiplies all of it by W:
// four times the pixels that carry information.  Here a block owns a 16 x 16 output tile, stages the 10 x 10
// source pixels its 18 x 18 ring samples ONCE (all Cin <= 256 channels, LDS-DMA), forms z_t for those pixels
// tap by tap with v_mfma_f32_16x16x32_f16 (128 rows: 100 pixels + padding), and blends z_t into fp32 output
// accumulators that live in registers across the nine taps.
//
// The x2 geometry.  With sc = (h - 1) / (2h - 1) the source pair of output coordinate o is
// i0 = floor(sc * o) = (o - 1) >> 1 (o >= 1; 0 for o = 0) and i1 = i0 + 1: the ring row k = o - (y0 - 1) of a
// tile at an even y0 reads the staged rows k >> 1 and (k >> 1) + 1, counted from source row y0 / 2 - 1, at
// every tile.  The slot indices are therefore compile-time constants and the blend's row sums stay in
// registers.  The WEIGHTS are not taken from that algebra: each ring row / column forms (i0, i1, w) with
// ac_coord, the resize kernel's own arithmetic, and gives slot s the weight [i0 == s] (1 - w) + [i1 == s] w
// (zero for a ring row / column outside the map: the conv's padding).  axis_ok checks on the host
// that the slots cover the pair of every output coordinate of the launch; a map where fp32 rounding breaks the
// pattern is not served.
//
// Block = 8 waves, persistent over tiles (halo_tile_of's order), one block per CU.  Per tap: ceil(Cin / 128) steps
// of two 64-channel K slabs each (32 MFMAs per wave; wave w = m-blocks 4 (w >> 2) .. + 3 x n-blocks 2 (w & 3), + 1),
// the weights of the next step streaming by LDS-DMA into a 2-slot ring (one wait + one raw s_barrier per step); then
// z_t -> LDS as fp16 (one extra rounding per tap, within the stage bar: tests/test_gpu_oc1_src.py; fp32 z would
// take the LDS the 128-channel steps use), a barrier, and the blend.  Blend thread = (output column, 4 channels),
// all 16 rows: per tap it blends the two staged columns of its ring column horizontally for each of the 10 staged
// rows (v_fma_mix_f32 off the packed fp16), summing the three taps of a tap row into one row-sum array, and after
// the third blends the row sums vertically into the 16 x 4 accumulators: 6 + 6 FMAs per output channel and tap row
// in place of 36.  The next tile's source pixels replace this tile's in place, slab by slab, as the last tap's
// steps release them; the tile ends waiting for them but not for its own output stores.
// LDS: x 64 KB and the W ring 2 x 32 KB (both as [128 rows][64 channels] blocks in vda_oc1.hip's weight layout),
// z 26 KB (100 pixels, row stride 264 B: conflict-free for the 8-B stores and the 256-B row reads).
//
// Measured (32 x 148^2 x 256 -> 296^2, profiles/oc1_src_*.log): 1216 us against the halo conv's 1777 us.  The
// timing-only ablations (VDA_OC1S_ABLATE) price the parts, each with the staging, the z stores, the barriers and
// the epilogue around it: MFMAs alone 818 us, blend alone 536 us, weight stream alone 806 us, MFMAs + weights
// 1060 us.  The parts run one after another within a block (lockstep steps), so what is left is their overlap: a
// deeper weight ring at 64-channel steps streams better (635 us alone) but its 36 barriers a tile cost the MFMA
// and blend phases more (1357 us in all), and a second z buffer to blend under the next tap's MFMAs does not fit
// beside 128-channel steps.
#include <cmath>
#include "vda_internal.h"
#include "vda_halo.h"

namespace {

__device__ __attribute__((aligned(64))) uint4 g_sz_page[4];

constexpr int ST = 16;               // output tile edge
constexpr int FP = 10;               // staged source rows / columns of a tile
constexpr int FPIX = FP * FP;        // 100
constexpr int MROWS = 128;           // MFMA rows (pixels, padded)
constexpr int CMAX = 256;            // input channels the x buffer holds
constexpr int CS = 64;               // input channels per step
constexpr int CO = 128;              // output channels
constexpr int CPX = CS / 8;          // 16-B chunks per weight row per step
constexpr int ZSTR = 132;            // halfs per z row (264 B)
constexpr int XBUF = MROWS * CMAX;   // halfs
constexpr int WBUF = CO * CS;        // halfs per weight ring slot
constexpr int ZBUF = FPIX * ZSTR;    // halfs: the window's pixels only (the padding rows' z is dropped)
constexpr int WPCS = CO * CPX / 64;  // weight pieces per step (16)
constexpr int WPW = WPCS / 8;        // per wave (2)
constexpr int SPS = 2;               // 64-channel slabs per step
constexpr int WSLOT = SPS * WBUF;    // halfs per weight ring slot
constexpr int WRING = 2;             // weight ring slots: a step's weights are fetched one step ahead

// timing-only ablations (SRC=vda_oc1_src tools/build_variants.sh name:"-DVDA_OC1S_ABLATE=n"; wrong results, never
// a route): 1 = no MFMAs and fragment reads, 2 = no blend, 4 = no weight stream
#ifndef VDA_OC1S_ABLATE
#define VDA_OC1S_ABLATE 0
#endif

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int w_pos(int n, int cd) { return cd ^ ((n >> 1) & (CPX - 1)); }

// weights of the two slots (source index g, g + 1) for output coordinate o of an `out`-long axis resized from `in`
__device__ __forceinline__ void slot_weights(int o, int out, int in, float sc, int g, float& a, float& b) {
  int i0, i1;
  float w;
  ac_coord(min(max(o, 0), out - 1), in, sc, i0, i1, w);
  const float u = 1.f - w;
  const bool ok = (unsigned)o < (unsigned)out;
  a = ok ? (i0 == g ? u : 0.f) + (i1 == g ? w : 0.f) : 0.f;
  b = ok ? (i0 == g + 1 ? u : 0.f) + (i1 == g + 1 ? w : 0.f) : 0.f;
}

__global__ __launch_bounds__(512) void oc1_src_kernel(const h16* __restrict__ x, const h16* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ b9,
                                                      h16* __restrict__ yout, int relu_out, int Hs, int Ws, int C,
                                                      int tiles_x, int tiles_y, int ntiles) {
  // separate arrays, not slices of one: the compiler orders an LDS access it sees behind every LDS-DMA in flight
  // unless the two name different variables, and the blend reads z while the weight ring is filling
  __shared__ __attribute__((aligned(16))) h16 xbuf[XBUF];
  __shared__ __attribute__((aligned(16))) h16 wbuf[WRING * WSLOT];
  __shared__ __attribute__((aligned(16))) h16 zbuf[ZBUF];
  __shared__ float2 vtab[ST + 2];  // the tile's vertical slot weights (block-uniform)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 3, mh = wave >> 2;
  const int frow = lane & 15, g = lane >> 4;
  const int H = 2 * Hs, W = 2 * Ws;
  const int nslab = C / CS;
  const int K = 9 * C;
  const int my_tiles = blockIdx.x < ntiles ? (ntiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  if (my_tiles == 0) return;
  const void* zero = (const void*)g_sz_page;
  const float usy = ac_scale(Hs, H), usx = ac_scale(Ws, W);

  // x in LDS: one [128 rows][64 channels] block per 64-channel slab, in the weight step's layout (row r's 16-B
  // chunk c at r * 8 + (c ^ ((r >> 1) & 7))); row = source pixel r * 10 + c of the tile's 10 x 10 window (rows
  // 100 .. 127 and pixels outside the map: zeros).  A slab is 16 pieces, two per wave, as a weight step is:
  // x_rows forms the two source pointers of this wave's rows once per tile (null: zeros), dma_x_step fetches a
  // step's slabs through them.  Slab s of the NEXT tile is fetched in place as soon as the last step that reads slab s
  // of this tile (tap 8, slab s) has passed its barrier.
  auto x_rows = [&](int bt, int y0, int x0, const h16* (&xp)[WPW]) {
    const int by = y0 / 2 - 1, bx = x0 / 2 - 1;
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
      const int s = (wave * WPW + j) * 64 + lane;
      const int row = s / CPX, cd = w_pos(row, s % CPX);
      const int r = row / FP, c = row - r * FP;
      const int gy = by + r, gx = bx + c;
      const bool ok = row < FPIX && (unsigned)gy < (unsigned)Hs && (unsigned)gx < (unsigned)Ws;
      xp[j] = ok ? x + (((long)bt * Hs + gy) * Ws + gx) * C + cd * 8 : nullptr;
    }
  };
  auto dma_x_step = [&](const h16* const (&xp)[WPW], int st) {  // always SPS * WPW pieces (the waits count them)
#pragma unroll
    for (int sub = 0; sub < SPS; ++sub) {
      const int slab = st * SPS + sub;
#pragma unroll
      for (int j = 0; j < WPW; ++j)
        glds16(xp[j] && slab < nslab ? (const void*)(xp[j] + slab * CS) : zero,
               xbuf + slab * WBUF + (wave * WPW + j) * 512);
    }
  };
  // The weight stream: step = (tap, SPS 64-channel slabs), 16 KB a slab (the layout of vda_oc1.hip), fetched one
  // step ahead of its use.  (pf_tile, pf_tap, pf_step) is the next step to fetch, pf_slot its ring slot; a step's
  // offset is a scalar added to two lane-constant row pointers.
  const h16* wrow[WPW];
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    const int s = (wave * WPW + j) * 64 + lane;
    const int n = s / CPX, pos = s - n * CPX;
    wrow[j] = w1 + (long)n * K + w_pos(n, pos) * 8;
  }
  const int nstep = (nslab + SPS - 1) / SPS;
  int pf_tile = 0, pf_tap = 0, pf_step = 0, pf_slot = 0;
  auto fetch_w = [&]() {  // false: no step left to fetch
    if (pf_tile >= my_tiles) return false;
#if !(VDA_OC1S_ABLATE & 4)
#pragma unroll
    for (int sub = 0; sub < SPS; ++sub) {
      const int slab = pf_step * SPS + sub;
      const unsigned off = (unsigned)(pf_tap * C + slab * CS);
#pragma unroll
      for (int j = 0; j < WPW; ++j)
        glds16(slab < nslab ? (const void*)(wrow[j] + off) : zero,
               wbuf + pf_slot * WSLOT + sub * WBUF + (wave * WPW + j) * 512);
    }
#endif
    if (++pf_step == nstep) {
      pf_step = 0;
      if (++pf_tap == 9) {
        pf_tap = 0;
        ++pf_tile;
      }
    }
    if (++pf_slot == WRING) pf_slot = 0;
    return true;
  };

  // lane-constant parts of the fragment addresses (LDS byte addresses: the fragment reads are asm)
  const int n0r = ng * 32 + frow;
  unsigned lin_w[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
    lin_w[d] = (unsigned)(uintptr_t)(VDA_LDS h16*)wbuf + (unsigned)(n0r * CPX + w_pos(n0r, d * 4 + g)) * 16u;
  unsigned lin_x[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
    lin_x[d] = (unsigned)(uintptr_t)(VDA_LDS h16*)xbuf +
               (unsigned)((mh * 64 + frow) * CPX + w_pos(mh * 64 + frow, d * 4 + g)) * 16u;
  // blend thread: output column xl, channels 4 cg .. + 3
  const int xl = tid >> 5, cg = tid & 31;

  const float* bsrc = b9 ? b9 + 4 * CO : b1;
  const f4 bias_r = bsrc ? *reinterpret_cast<const f4*>(bsrc + cg * 4) : f4{0.f, 0.f, 0.f, 0.f};

  float acc[ST][4];
#pragma unroll
  for (int i = 0; i < ST; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;

  int bt, y0, x0;
  halo_tile_of(blockIdx.x, tiles_x, tiles_y, ST, bt, y0, x0);
  const h16* nxp[WPW];  // this wave's source pointers of the next tile
  x_rows(bt, y0, x0, nxp);
  for (int st = 0; st < nstep; ++st) dma_x_step(nxp, st);
#pragma unroll
  for (int k = 0; k < WRING - 1; ++k) fetch_w();
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();

  int rd_slot = 0;  // the weight ring slot of the current step
  for (int ti = 0; ti < my_tiles; ++ti) {
    const bool more = ti + 1 < my_tiles;
    int nbt = 0, ny0 = 0, nx0 = 0;
    if (more) halo_tile_of(blockIdx.x + (ti + 1) * gridDim.x, tiles_x, tiles_y, ST, nbt, ny0, nx0);
    // vertical slot weights of the 18 ring rows (block-uniform) -> vtab, published by the first step's barrier
    // (the previous tile's last reads of it precede the barrier that ends that tile); horizontal ones of this
    // thread's three ring columns
    if (tid < ST + 2) {
      float a, b;
      slot_weights(y0 - 1 + tid, H, Hs, usy, y0 / 2 - 1 + (tid >> 1), a, b);
      vtab[tid] = make_float2(a, b);
    }
    float hA[3], hB[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
      slot_weights(x0 - 1 + xl + tx, W, Ws, usx, x0 / 2 - 1 + ((xl + tx) >> 1), hA[tx], hB[tx]);

    float hs[FP][4];  // row sums of one tap row
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ty = tap / 3, tx = tap % 3;
      f4 za[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) za[a][i] = f4{0.f, 0.f, 0.f, 0.f};
      if (tap == 8 && more) x_rows(nbt, ny0, nx0, nxp);
      for (int st = 0; st < nstep; ++st) {
        fetch_w();
        // the x slabs of the previous step, which nobody reads again: the next tile's, in place, AFTER this
        // step's weights in the queue, so that the wait below can leave them in flight
        const bool xs = tap == 8 && more && st > 0;
        if (xs) dma_x_step(nxp, st - 1);
#if !(VDA_OC1S_ABLATE & 1)
        // Fragment reads as asm: a compiler-visible LDS read gets an s_waitcnt vmcnt(0) in front of it while an
        // LDS-DMA that may alias it is in flight, which here is the weight stream itself.
        // Per k-depth the six reads are issued and waited for by a wait that carries the fragment registers, so
        // the MFMAs cannot move above it; the SIMD's other wave covers the read latency.
#pragma unroll
        for (int d = 0; d < 2 * SPS; ++d) {
          const int slab = st * SPS + (d >> 1);
          if (slab < nslab) {
            const unsigned wa = lin_w[d & 1] + rd_slot * (WSLOT * 2) + (d >> 1) * (WBUF * 2);
            const unsigned xa = lin_x[d & 1] + slab * (WBUF * 2);
            u32x4 wf[2], xf[4];
#pragma unroll
            for (int a = 0; a < 2; ++a)
              asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[a]) : "v"(wa), "n"(a * 16 * CPX * 16));
#pragma unroll
            for (int i = 0; i < 4; ++i)
              asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xf[i]) : "v"(xa), "n"(i * 16 * CPX * 16));
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(wf[0]), "+v"(wf[1]), "+v"(xf[0]), "+v"(xf[1]), "+v"(xf[2]), "+v"(xf[3]));
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                za[a][i] = mfma16(__builtin_bit_cast(h8, wf[a]), __builtin_bit_cast(h8, xf[i]), za[a][i]);
          }
        }
#endif
        // the next step's weights have landed; in the last tap the x pieces issued after them may stay in flight
        if (xs) wait_vmcnt<SPS * WPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        rd_slot ^= 1;
      }
      if (tap == 8 && more) dma_x_step(nxp, nstep - 1);
      // z_t -> LDS, fp16: a lane holds channels (2 ng + a) 16 + 4 g .. + 3 of pixel (4 mh + i) 16 + frow.  asm
      // stores: a compiler-visible LDS store that may alias the LDS-DMA destinations gets an s_waitcnt
      // vmcnt(0) in front of it (vda_oc1.hip)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          typedef float f2v __attribute__((ext_vector_type(2)));
          const f4 v = za[a][i];
          const u32x2 o = {__builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[0], v[1]}, h2)),
                           __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{v[2], v[3]}, h2))};
          const int pix = (mh * 4 + i) * 16 + frow;
          const h16* dst = zbuf + pix * ZSTR + (ng * 2 + a) * 16 + g * 4;
          if (pix < FPIX)
            asm volatile("ds_write_b64 %0, %1" ::"v"((unsigned)(uintptr_t)(VDA_LDS h16*)dst), "v"(o) : "memory");
        }
      lgkm0();
      __builtin_amdgcn_s_barrier();
#if !(VDA_OC1S_ABLATE & 2)
      // horizontal: row sums of the tap row, += the blend of the two staged columns of ring column xl + tx
      {
        // the thread's z address is re-formed from an opaque copy of its id per tap: hoisted, the three tap
        // columns' addresses are spilled, and a scratch reload waits on vmcnt, i.e. on the weight stream
        int t = tid;
        asm volatile("" : "+v"(t));
        const h16* zc = zbuf + (((t >> 5) + tx) >> 1) * ZSTR + (t & 31) * 4;
        const float wa = hA[tx], wb2 = hB[tx];
#pragma unroll
        for (int r = 0; r < FP; ++r) {
          if (r < (ty >> 1) || r > ((ST - 1 + ty) >> 1) + 1) continue;  // rows this tap row never blends
          const uint2 p = *reinterpret_cast<const uint2*>(zc + r * FP * ZSTR);
          const uint2 q = *reinterpret_cast<const uint2*>(zc + r * FP * ZSTR + ZSTR);
          const float s0 = tx == 0 ? 0.f : hs[r][0], s1 = tx == 0 ? 0.f : hs[r][1];
          const float s2 = tx == 0 ? 0.f : hs[r][2], s3 = tx == 0 ? 0.f : hs[r][3];
          hs[r][0] = fma_mix_lo(wb2, q.x, fma_mix_lo(wa, p.x, s0));
          hs[r][1] = fma_mix_hi(wb2, q.x, fma_mix_hi(wa, p.x, s1));
          hs[r][2] = fma_mix_lo(wb2, q.y, fma_mix_lo(wa, p.y, s2));
          hs[r][3] = fma_mix_hi(wb2, q.y, fma_mix_hi(wa, p.y, s3));
        }
      }
      // vertical, after the tap row's third tap: output row i reads ring row i + ty
      if (tx == 2) {
#pragma unroll
        for (int i = 0; i < ST; ++i) {
          const int k = i + ty;
          const float2 vw = vtab[k];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[i][c] = __builtin_fmaf(vw.y, hs[(k >> 1) + 1][c], __builtin_fmaf(vw.x, hs[k >> 1][c], acc[i][c]));
        }
        // The accumulators are made opaque here: they start a tile at zero and only the epilogue reads them, so
        // the compiler otherwise sinks all three vertical passes into the epilogue and keeps 3 x 40 row sums
        // alive (and spilled) in place of 64 accumulators.
#pragma unroll
        for (int i = 0; i < ST; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(acc[i][c]));
      }
#endif
    }
    // epilogue: + bias (class row on the map's outer ring) [ReLU] -> fp16.  A thread holds 4 channels of 16 rows;
    // the lane pair (cg, cg ^ 1) trades halves of each row pair so that the even lane stores 8 channels (16 B) of
    // the even row and the odd lane of the odd row: 32 lanes = two pixels' 256 B, half the store instructions of
    // 8-B pieces.  Pixels outside the map are dropped by the buffer's range check.
    {
      const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(yout + (long)bt * H * W * CO), (short)0, (int)((long)H * W * CO * 2), 0x00020000);
      const bool ring = b9 != nullptr && (y0 == 0 || y0 + ST >= H || x0 == 0 || x0 + ST >= W);  // block-uniform
      const int xg = x0 + xl;
      const bool odd = (cg & 1) != 0;
#pragma unroll
      for (int i = 0; i < ST; i += 2) {
        u32x2 o[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int yg = y0 + i + e;
          f4 bv = bias_r;
          if (ring) {
            const int cls = (yg == 0 ? 0 : yg >= H - 1 ? 2 : 1) * 3 + (xg == 0 ? 0 : xg >= W - 1 ? 2 : 1);
            bv = *reinterpret_cast<const f4*>(b9 + cls * CO + cg * 4);
          }
          h4 h;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float v = acc[i + e][c] + bv[c];
            h[c] = (h16)(relu_out ? fmaxf(v, 0.f) : v);
            acc[i + e][c] = 0.f;
          }
          o[e] = __builtin_bit_cast(u32x2, h);
        }
        const u32x2 snd = odd ? o[0] : o[1];
        u32x2 rcv;  // the partner lane's `snd` (quad_perm [1, 0, 3, 2])
        rcv[0] = (unsigned)__builtin_amdgcn_mov_dpp((int)snd[0], 0xB1, 0xF, 0xF, true);
        rcv[1] = (unsigned)__builtin_amdgcn_mov_dpp((int)snd[1], 0xB1, 0xF, 0xF, true);
        const u32x4 val = odd ? u32x4{rcv[0], rcv[1], o[1][0], o[1][1]} : u32x4{o[0][0], o[0][1], rcv[0], rcv[1]};
        const int yg = y0 + i + (odd ? 1 : 0);
        const unsigned vo = (yg < H && xg < W) ? (unsigned)(((yg * W + xg) * CO + (cg & ~1) * 4) * 2) : 0x80000000u;
        __builtin_amdgcn_raw_buffer_store_b128(val, ys, vo, 0, 0);
      }
    }
    if (more) {
      bt = nbt; y0 = ny0; x0 = nx0;
      // the next tile's x has landed (its last slab is older than this tile's stores, which stay in flight: ST / 2
      // a lane, and on a ring tile its class-row loads)
      wait_vmcnt<ST / 2>();
      __builtin_amdgcn_s_barrier();
    }
  }
}

// Do the two staged slots of every ring row / column cover the source pair ac_coord forms for it?  In exact
// arithmetic always; in fp32 the product sc * o can fall just under an integer (the last coordinate, sc * (2n - 1)
// = n - 1), which moves weight <= a few ulp to a row outside the slots.  A coordinate that loses more is refused.
bool axis_ok(int n) {
  const float sc = ac_scale(n, 2 * n);
  for (int o = 0; o < 2 * n; ++o) {
    const float f = sc * (float)o;
    const int i0 = (int)f, i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    const float w = std::fmaf(sc, (float)o, -(float)i0);
    const int ga = ((o + 1) >> 1) - 1;
    const float kept = (i0 == ga || i0 == ga + 1 ? 1.f - w : 0.f) + (i1 == ga || i1 == ga + 1 ? w : 0.f);
    if (!(kept > 1.f - 1e-5f)) return false;
  }
  return true;
}

}  // namespace

// vda_debug_oc1_src (tuning build): 1 = automatic: the source-resolution kernel for the conv with a bias9 table (the
// composed out_conv . output_conv1, which has no materialised counterpart), the halo conv with the fused resize
// (vda_oc1.hip), whose bits are those of resize + conv, for a plain bias; 2 = the source-resolution kernel wherever
// it serves; 0 = never
VDA_KNOB(int, g_oc1_src, 1);

// Serves exactly the x2 resize (H, W) = (2 Hs, 2 Ws), Cin % 64 == 0 up to the 256 channels its x buffer holds,
// Cout == 128
bool vda_conv_oc1_src_serves(int BT, int Hs, int Ws, int H, int W, int Cin, int Cout, bool bias9) {
  if (!(g_oc1_src == 2 || (g_oc1_src == 1 && bias9)) || Cout != CO || Cin % CS != 0 || Cin > CMAX || BT < 1 || Hs < 1 || Ws < 1) return false;
  if (H != 2 * Hs || W != 2 * Ws) return false;
  if ((long)H * W * Cout * 2 >= (1L << 31)) return false;  // per-frame buffer stores take 32-bit offsets
  HaloGrid g;
  if (!halo_tile_grid(BT, H, W, ST, 1, 0x7fffffffL, g)) return false;
  return axis_ok(Hs) && axis_ok(Ws);
}

int vda_conv_oc1_src(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int Hs, int Ws, int H,
                     int W, int Cin, int Cout, hipStream_t st, const float* bias9) {
  if (!vda_conv_oc1_src_serves(BT, Hs, Ws, H, W, Cin, Cout, bias9 != nullptr)) return 1;
  HaloGrid g;
  halo_tile_grid(BT, H, W, ST, 1, 0x7fffffffL, g);
  hipLaunchKernelGGL(oc1_src_kernel, dim3(g.grid), dim3(512), 0, st, (const h16*)x, (const h16*)w, bias, bias9,
                     (h16*)y, relu, Hs, Ws, Cin, g.tiles_x, g.tiles_y, g.ntiles);
  VDA_LAUNCH_CHECK();
  return 0;
}

#ifdef VDA_TUNING
extern "C" int vda_debug_oc1_src(int32_t mode) {
  if (mode < 0 || mode > 2) return 1;
  g_oc1_src = mode;
  return 0;
}
#endif
