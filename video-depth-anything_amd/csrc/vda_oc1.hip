// output_conv1 as a halo-tiled conv (dpt.py:117): a 3x3 / stride 1 / pad 1 conv Cin -> 128 (Cin % 64 == 0),
// epilogue +bias [ReLU] -> fp16 NHWC, on a map x [BT, H, W, Cin] fp16 or (UPS) on the bilinear
// (align_corners=True) resize of x [BT, Hs, Ws, Cin] to (H, W), which is then never written to HBM.
//
// Why a halo tile: the implicit-GEMM conv re-reads every input pixel once per tap (9x).  Here a block owns
// a 16x16 output tile and stages the 18x18-pixel input patch ONCE per 64-channel slab (LDS-DMA), then runs
// all 9 taps out of LDS: input traffic 1.27x the map instead of 9x, weights streamed per (slab, tap) step
// (16 KB) from L2.
//
// Block = 8 MFMA waves, persistent over tiles.  Wave w: output rows 4*(w&3) .. +3 of the tile (4 m-blocks
// of 16 pixels) x n-blocks 4*(w>>2) .. +3 (64 of the 128 output channels).  Pipeline: 2 patch slabs (ring)
// and 2 weight steps (ring); per step (one tap: 32 MFMAs per wave) each wave issues the next step's weight
// pieces, and on a unit's first step the whole next patch slab; the counted end-of-step vmcnt leaves only
// those patch pieces in flight; one raw s_barrier per step.  LDS layouts: the patch is linear in the pixel
// with the pixel stride padded to PSTR = 10 16-B slots (8 hold the slab's channels), so a tap moves every
// fragment read by one constant: per step the reads cost one address add per output row and the rest are
// immediates; weights row*8 + (chunk ^ ((row >> 1) & 7)).  Both are conflict-free for the ds_read_b128
// lane groups at any patch offset (brute-forced).
//
// UPS: the source region a tile's 18x18 patch needs (<= HALO_SRC_PIXELS pixels, halo_fused_fits) is staged
// per slab by LDS-DMA into its own slot, and the patch is interpolated from it in fp32 with the resize
// kernel's formula and op order, so the fp16 values are bit-identical to a materialised resize.  4 extra
// interpolation waves (8 .. 11) own the staging and the interpolation: they fetch unit u+1's source region
// at steps 0-1 of unit u and build its patch over the following steps (ups_interp_item, 256 items a step)
// beside the 8 MFMA waves' taps, which then never stop for the interpolation; every wave takes every step
// barrier.  Only unit 0's patch is built by the MFMA waves, in the prologue (ups_interp).
#include "vda_internal.h"
#include "vda_halo.h"

namespace {

__device__ __attribute__((aligned(64))) uint4 g_dz_page[4];
#ifdef VDA_TS  // per-block step-class cycle sums of output_conv1 (tools/ts_oc1.py; experiments only)
__device__ unsigned long long g_dts[1024][24];
#endif

constexpr int DT = 16;              // output tile edge
constexpr int DP = DT + 2;          // patch edge (halo 1)
constexpr int DNPIX = DP * DP;      // 324
constexpr int CS = 64;              // input channels per slab (one pipeline unit)
constexpr int CO = 128;             // output channels
constexpr int NB = CO / 32;         // n-blocks per wave
constexpr int CPX = CS / 8;         // 16-B chunks per pixel per slab
constexpr int PSTR = 10;            // 16-B slots per patch pixel (padded: see the header)
constexpr int ND = CS / 32;         // MFMA k-depths per tap
constexpr int SPU = 9;              // steps per unit: one tap each

typedef unsigned dh_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int w_pos(int n, int cd) { return cd ^ ((n >> 1) & (CPX - 1)); }

template <bool UPS>
__global__ __launch_bounds__(UPS ? 768 : 512) void halo_conv_kernel(const h16* __restrict__ U, const h16* __restrict__ w1,
                                                                  const float* __restrict__ b1, h16* __restrict__ yout,
                                                                  int relu_out, int H, int W, int C, int tiles_x,
                                                                  int tiles_y, int ntiles, int Hs = 0, int Ws = 0,
                                                                  const float* __restrict__ b9 = nullptr) {
  constexpr int IW = UPS ? 4 : 0;                        // interpolation waves
  constexpr int PSLOT = DNPIX * PSTR;                    // 16-B slots of one patch slab
  constexpr int PP = (PSLOT + 63) / 64;                  // 1-KiB DMA pieces per slab
  constexpr int PBUF = (UPS ? PSLOT : PP * 64) * 8;      // halfs per patch ring slot
  constexpr int WSLOT = CO * CPX;                        // 16-B slots of one weight step
  constexpr int WBUF = WSLOT * 8;                        // halfs
  constexpr int WPCS = WSLOT / 64;                       // weight pieces per step (16)
  constexpr int WPW = (WPCS + 7) / 8;                    // per wave (2)
  constexpr int WRING = 2;                               // weight ring
  constexpr int SPPW = (HALO_SRC_PIXELS * CPX + 511) / 512;  // UPS source pieces per wave (fixed count)
  constexpr int SSLOT = UPS ? SPPW * 8 * 64 : 0;         // source slots: every pixel halo_fused_fits admits
  static_assert(SPPW * 8 * 64 >= HALO_SRC_PIXELS * CPX, "source slot: HALO_SRC_PIXELS pixels x CPX chunks");
  __shared__ __attribute__((aligned(16))) h16 dsm[2 * PBUF + WRING * WBUF + SSLOT * 8];
  h16* patch = dsm;                                      // [2][PBUF]
  h16* wbuf = dsm + 2 * PBUF;                            // [WRING][WBUF]
  h16* sbuf = dsm + 2 * PBUF + WRING * WBUF;             // [SSLOT * 8] (UPS)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mg = wave & 3, ng = wave >> 2;
  const bool iwave = IW > 0 && wave >= 8;                // interpolation wave (no MFMA work)
  const int nslab = C / CS;
  const int K = 9 * C;
  const int units_per_tile = nslab;
  // tiles of this block: t = blockIdx.x + i * gridDim.x
  const int my_tiles = blockIdx.x < ntiles ? (ntiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  const int my_units = my_tiles * units_per_tile;
  if (my_units == 0) return;
  const int my_steps = my_units * SPU;
  const void* zero = (const void*)g_dz_page;

  // a unit's coordinates are formed once (the divisions are scalar but long), not per DMA piece
  struct Ud { int bt, y0, x0, slab, sy_lo, sx_lo, SR, SC; };
  auto tile_of_unit = [&](int u, int& bt, int& y0, int& x0) {
    halo_tile_of(blockIdx.x + (u / units_per_tile) * gridDim.x, tiles_x, tiles_y, DT, bt, y0, x0);
  };
  // piece q of unit u's patch slab -> ring slot (u & 1)
  auto dma_patch = [&](int u, const Ud& ud, int q) {
    const int bt = ud.bt, y0 = ud.y0, x0 = ud.x0, slab = ud.slab;
    const int s = q * 64 + lane;
    const int p = s / PSTR, cd = s - p * PSTR;
    const int pr = p / DP;
    const int py = y0 - 1 + pr, px = x0 - 1 + (p - pr * DP);
    const void* src = zero;
    if (p < DNPIX && cd < CPX && (unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W)
      src = U + (((long)bt * H + py) * W + px) * C + slab * CS + cd * 8;
    glds16(src, patch + (u & 1) * PBUF + q * 512);
  };
  // UPS: a unit's Ud holds the source region of its patch (halo_src_region): rows sy_lo .. sy_lo + SR - 1,
  // columns sx_lo .. + SC - 1
  constexpr int USL = DNPIX * CPX;                       // 16-B patch slots read by the taps
  constexpr int UCH = UPS ? (USL + 511) / 512 : 1;       // patch slots per thread
  const float usy = UPS ? ac_scale(Hs, H) : 0.f, usx = UPS ? ac_scale(Ws, W) : 0.f;
  auto make_ud = [&](int u) {
    Ud ud;
    tile_of_unit(u, ud.bt, ud.y0, ud.x0);
    ud.slab = u % units_per_tile;
    ud.sy_lo = ud.sx_lo = ud.SR = ud.SC = 0;
    if constexpr (UPS) halo_src_region(usy, usx, ud.y0, ud.x0, DT, H, W, Hs, Ws, ud.sy_lo, ud.sx_lo, ud.SR, ud.SC);
    return ud;
  };
  // piece q of a unit's source region -> sbuf; slot = pixel * CPX + chunk
  auto dma_src = [&](const Ud& ud, int q) {
    const int bt = ud.bt, sy_lo = ud.sy_lo, sx_lo = ud.sx_lo, SR = ud.SR, SC = ud.SC, slab = ud.slab;
    const int s = q * 64 + lane;
    const int px = s / CPX, cd = s % CPX;
    const int r = px / SC, c = px - r * SC;
    const void* src = zero;
    if (r < SR) src = U + (((long)bt * Hs + sy_lo + r) * Ws + sx_lo + c) * C + slab * CS + cd * 8;
    glds16(src, sbuf + q * 512);
  };
  // interpolate unit u's patch from sbuf into patch ring slot (u & 1); padding pixels -> 0
  // slots t0 + k * tstride (k < NK) of the patch (t0 = this thread's first)
  auto ups_interp = [&](int u, const Ud& ud, int t0, int tstride, auto nk_tag) {
    constexpr int NK = decltype(nk_tag)::value;
    const int y0 = ud.y0, x0 = ud.x0, sy_lo = ud.sy_lo, sx_lo = ud.sx_lo, SC = ud.SC;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int s = t0 + k * tstride;
      const int sc = min(s, USL - 1);
      const int p = sc / CPX, cd = sc - p * CPX;
      const int pr = p / DP;
      const int py = y0 - 1 + pr, px = x0 - 1 + (p - pr * DP);
      const bool ok = (unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W;
      int sy0, sy1, sx0, sx1;
      float wy, wx;
      ac_coord(min(max(py, 0), H - 1), Hs, usy, sy0, sy1, wy);
      ac_coord(min(max(px, 0), W - 1), Ws, usx, sx0, sx1, wx);
      const int r0 = (sy0 - sy_lo) * SC, r1 = (sy1 - sy_lo) * SC, c0 = sx0 - sx_lo, c1 = sx1 - sx_lo;
      const h8 a = *reinterpret_cast<const h8*>(sbuf + ((r0 + c0) * CPX + cd) * 8);
      const h8 b = *reinterpret_cast<const h8*>(sbuf + ((r0 + c1) * CPX + cd) * 8);
      const h8 c = *reinterpret_cast<const h8*>(sbuf + ((r1 + c0) * CPX + cd) * 8);
      const h8 d = *reinterpret_cast<const h8*>(sbuf + ((r1 + c1) * CPX + cd) * 8);
      const h8 v = bilerp8(a, b, c, d, wx, wy);
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      const uint4 o = ok ? __builtin_bit_cast(uint4, v) : z;
      const int slot = p * PSTR + cd;
      // asm store: a compiler-visible LDS store that may alias the LDS-DMA ring gets an s_waitcnt
      // vmcnt(0) in front of it, which drained the next step's weight DMA before the interpolation
      if (s < USL)
        asm volatile("ds_write_b128 %0, %1" ::"v"((unsigned)(uintptr_t)(VDA_LDS h16*)(patch + (u & 1) * PBUF + slot * 8)),
                     "v"(__builtin_bit_cast(dh_u4, o))
                     : "memory");
    }
    lgkm0();  // the stores above are invisible to the compiler's counts
  };
  // The interpolation waves' form of ups_interp: item = (patch column, channel chunk, ISEG-row segment)
  // of halo_blend_column, stored with the asm ds_write_b128 (as above)
  constexpr int ISEG = 3;                                // rows per item (6: 1809, 9: 1966 vs 1781 us)
  constexpr int NITEM = (DP / ISEG) * DP * CPX;          // 432 for a 64-channel slab
  auto ups_interp_item = [&](int u, const Ud& ud, int it) {
    if (it >= NITEM) return;
    const int SC = ud.SC;
    const int cd = it % CPX, col = (it / CPX) % DP, seg = it / (CPX * DP);
    halo_blend_column<ISEG>(
        usy, usx, ud.y0, ud.x0, col, seg * ISEG, H, W, Hs, Ws, ud.sy_lo, ud.sx_lo,
        [&](int r, int c) { return *reinterpret_cast<const uint4*>(sbuf + ((r * SC + c) * CPX + cd) * 8); },
        [&](int pr, uint4 v) {
          const int slot = (pr * DP + col) * PSTR + cd;
          asm volatile("ds_write_b128 %0, %1" ::"v"((unsigned)(uintptr_t)(VDA_LDS h16*)(patch + (u & 1) * PBUF + slot * 8)),
                       "v"(__builtin_bit_cast(dh_u4, v))
                       : "memory");
        });
    lgkm0();  // the asm stores are invisible to the compiler's counts
  };
  // weight pieces of step st (= tap) of a unit of slab `slab` -> ring slot `wslot`
  auto dma_w = [&](int st, int slab, int wslot) {
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
      const int piece = (wave * WPW + j) % WPCS;
      const int s = piece * 64 + lane;
      const int n = s / CPX, pos = s - n * CPX;
      const int cd = w_pos(n, pos);
      glds16(w1 + (long)n * K + st * C + slab * CS + cd * 8, wbuf + wslot * WBUF + piece * 512);
    }
  };

  // prologue: patch of unit 0 (all pieces, split over waves) + weights of step 0
  Ud ud_next = make_ud(0);
  if constexpr (UPS) {
    if (!iwave) {
      for (int j = 0; j < SPPW; ++j) dma_src(ud_next, wave + j * 8);
      dma_w(0, ud_next.slab, 0);
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (!iwave) ups_interp(0, ud_next, tid, 512, std::integral_constant<int, UCH>{});
    __syncthreads();  // patch slot 0 written, source slot free for unit 1
  } else {
    for (int q = wave; q < PP; q += 8) dma_patch(0, ud_next, q);
    dma_w(0, ud_next.slab, 0);
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();

  if constexpr (UPS) {
    if (iwave) {
      // the interpolation waves' own step loop (same barrier sequence as the MFMA waves' loop below, no
      // accumulators live): unit u+1's source region in two halves at steps 0 and 1 (waited for before
      // step 2's barrier; all at step 0 and blending from step 2: 1820 vs 1784 us), its patch items over
      // steps 3 .. 2 + ISTEPS (64 IW a step); the step barriers publish the writes
      constexpr int SPI = SPPW * 8 / IW;                 // source pieces per interpolation wave
      constexpr int ISTEPS = (NITEM + 64 * IW - 1) / (64 * IW);
      static_assert(SPPW * 8 % IW == 0 && ISTEPS <= SPU - 3, "interpolation wave split");
      int iu = 0, ist = 0;
      for (int gs = 0; gs < my_steps; ++gs) {
        if (ist == 0 && iu + 1 < my_units) {
          ud_next = make_ud(iu + 1);
          for (int j = 0; j < SPI / 2; ++j) dma_src(ud_next, (wave - 8) + j * IW);
        }
        if (ist == 1 && iu + 1 < my_units)
          for (int j = SPI / 2; j < SPI; ++j) dma_src(ud_next, (wave - 8) + j * IW);
        if (ist >= 3 && ist < 3 + ISTEPS && iu + 1 < my_units)
          ups_interp_item(iu + 1, ud_next, (ist - 3) * 64 * IW + (tid - 512));
        if (ist == 2) wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (++ist == SPU) {
          ist = 0;
          ++iu;
        }
      }
      return;
    }
  }
  const int frow = lane & 15, g = lane >> 4;
  // lane-constant byte offsets of the fragment reads (output row i, k-depth d and the tap are
  // immediates / one scalar per step); W rows keep their XOR swizzle, which depends on the row only
  const unsigned lin_x = (unsigned)(((mg * 4) * DP + frow) * PSTR + g) * 16u;
  unsigned lin_w[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const int n0r = ng * NB * 16 + frow;
    lin_w[d] = (unsigned)(n0r * CPX + w_pos(n0r, d * 4 + g)) * 16u;
  }
  f4 acc[NB][4];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[a][i] = f4{0.f, 0.f, 0.f, 0.f};
  // the bias, held for the whole launch (a lane's channels do not change with the tile): a load in the
  // epilogue made every tile end wait (vmcnt(0)) for it.  With a 9-class table b9 [9][CO] (vda_epilogue.bias9)
  // the registers hold the middle class, which serves every tile off the map's outer ring; a tile that touches
  // the ring loads each pixel's class row in its epilogue.
  const float* bsrc = b9 ? b9 + 4 * CO : b1;
  f4 bias_r[NB];
#pragma unroll
  for (int a = 0; a < NB; ++a)
    bias_r[a] = bsrc ? *reinterpret_cast<const f4*>(bsrc + (ng * NB + a) * 16 + g * 4) : f4{0.f, 0.f, 0.f, 0.f};
  const int my_pp = (PP - 1 - wave) / 8 + 1;             // next-slab patch pieces of this wave
  constexpr int PPMAX = (PP + 7) / 8;

  // step counters kept incrementally (no per-step division): unit u, its step st and slab
  int u = 0, st = 0, slab = 0;
#ifdef VDA_TS
  // class = step within the unit (0..SPU-1), SPU = a tile's last step; sums of s_memtime deltas between
  // consecutive end-of-step barriers (and of the end-of-step wait + barrier alone), taken by every wave
  // (uniform), stored by thread 0 at the end
  unsigned long long tsa[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned tsn[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long ts_rt0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long ts_c0 = __builtin_amdgcn_s_memtime();
  unsigned long long ts_prev = ts_c0, tsw = 0;
#endif
  for (int gs = 0; gs < my_steps; ++gs) {
    // weights of the next step first, then (first step of a unit) the whole next patch slab: the
    // end-of-step wait then leaves exactly the patch pieces in flight, and they land by the end of
    // the unit's second step.  UPS: the interpolation waves build the next patch instead.
    const bool issue_p = st == 0 && u + 1 < my_units;
    if (issue_p) ud_next = make_ud(u + 1);
    if (gs + 1 < my_steps) {
      if (st + 1 < SPU) dma_w(st + 1, slab, (gs + 1) & 1);
      else dma_w(0, slab + 1 == nslab ? 0 : slab + 1, (gs + 1) & 1);
    }
    if constexpr (!UPS) {
      if (issue_p)
        for (int j = 0; j < my_pp; ++j) dma_patch(u + 1, ud_next, wave + j * 8);
    }
    // ---- one tap: ND k-depths x (NB x 4) MFMAs
    {
      // one scalar per step: patch slot + this step's tap offset, W slot (opaque: no strength
      // reduction of the modulo counters into per-read VALU)
      const h16* pb = patch + (u & 1) * PBUF;  // this step's ring slots
      const h16* wb = wbuf + (gs & 1) * WBUF;
      unsigned xs, ws;
      asm volatile("s_mov_b32 %0, %1" : "=s"(xs)
                   : "s"((unsigned)((pb - patch) * 2 + ((st / 3) * DP + (st % 3)) * PSTR * 16)));
      asm volatile("s_mov_b32 %0, %1" : "=s"(ws) : "s"((unsigned)((wb - wbuf) * 2)));
      const char* pxb = reinterpret_cast<const char*>(patch) + xs + lin_x;
      const char* wxb[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) wxb[d] = reinterpret_cast<const char*>(wbuf) + ws + lin_w[d];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        h8 wf[NB], xf[4];
#pragma unroll
        for (int a = 0; a < NB; ++a) wf[a] = *reinterpret_cast<const h8*>(wxb[d] + a * 16 * CPX * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = *reinterpret_cast<const h8*>(pxb + i * DP * PSTR * 16 + d * 64);
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[a][i] = mfma16(wf[a], xf[i], acc[a][i]);
      }
    }
    const bool tile_end = st == SPU - 1 && slab == units_per_tile - 1;
    if (tile_end) {
      // +bias [ReLU] -> fp16 NHWC.  A lane holds 4 consecutive channels of pixel (row mg*4+i, col frow)
      // per n-block; lane groups g and g^1 (lanes l, l^16) trade one n-block of each pair so that every
      // lane stores 8 consecutive channels (16 B: half the store instructions of 8-B pieces).  Buffer
      // stores over the frame, pixels outside the map dropped by the range check, so every lane issues
      // exactly NB / 2 * 4 of them (the end-of-step wait below counts them).
      int bt, y0, x0;
      tile_of_unit(u, bt, y0, x0);
      const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(yout + (long)bt * H * W * CO), (short)0, (int)((long)H * W * CO * 2), 0x00020000);
      const bool godd = (g & 1) != 0;
      const bool ring = b9 != nullptr && (y0 == 0 || y0 + DT >= H || x0 == 0 || x0 + DT >= W);  // block-uniform
#pragma unroll
      for (int a = 0; a < NB; a += 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int y = y0 + mg * 4 + i, x = x0 + frow;
          f4 bv0 = bias_r[a], bv1 = bias_r[a + 1];
          if (ring) {  // pixels past the map (dropped by the store) take some class's row: the table has 9
            const int cls = (y == 0 ? 0 : y >= H - 1 ? 2 : 1) * 3 + (x == 0 ? 0 : x >= W - 1 ? 2 : 1);
            const float* bp = b9 + cls * CO + (ng * NB + a) * 16 + g * 4;
            bv0 = *reinterpret_cast<const f4*>(bp);
            bv1 = *reinterpret_cast<const f4*>(bp + 16);
          }
          const f4 v0 = acc[a][i] + bv0, v1 = acc[a + 1][i] + bv1;
          h4 o0, o1;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o0[r] = (h16)(relu_out ? fmaxf(v0[r], 0.f) : v0[r]);
            o1[r] = (h16)(relu_out ? fmaxf(v1[r], 0.f) : v1[r]);
          }
          const uint2 u0 = __builtin_bit_cast(uint2, o0), u1 = __builtin_bit_cast(uint2, o1);
          const uint2 snd = godd ? u0 : u1;
          float ax, bx, ay, by;
          swap16_pair(__builtin_bit_cast(float, snd.x), ax, bx);
          swap16_pair(__builtin_bit_cast(float, snd.y), ay, by);
          const uint2 rcv = make_uint2(__builtin_bit_cast(unsigned, godd ? ax : bx), __builtin_bit_cast(unsigned, godd ? ay : by));
          const u32x4 val = godd ? u32x4{rcv.x, rcv.y, u1.x, u1.y} : u32x4{u0.x, u0.y, rcv.x, rcv.y};
          const int n = (ng * NB + a + (godd ? 1 : 0)) * 16 + (g & 2) * 4;
          const unsigned vo = (y < H && x < W) ? (unsigned)(((y * W + x) * CO + n) * 2) : 0x80000000u;
          __builtin_amdgcn_raw_buffer_store_b128(val, ys, vo, 0, 0);
          acc[a][i] = f4{0.f, 0.f, 0.f, 0.f};
          acc[a + 1][i] = f4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
#ifdef VDA_TS
    const unsigned long long ts_pre = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (UPS) {
      if (tile_end) wait_vmcnt<NB / 2 * 4>();  // the next step's weights, not the tile's stores
      else wait_vmcnt<0>();
    } else if (issue_p) {
      if (my_pp == PPMAX) wait_vmcnt<PPMAX>();
      else wait_vmcnt<PPMAX - 1>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
#ifdef VDA_TS
    {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      const int cls = tile_end ? SPU : st;
#pragma unroll
      for (int c = 0; c <= SPU && c < 10; ++c)
        if (c == cls) { tsa[c] += now - ts_prev; ++tsn[c]; }
      tsw += now - ts_pre;
      ts_prev = now;
    }
#endif
    if (++st == SPU) {
      st = 0;
      ++u;
      if (++slab == nslab) slab = 0;
    }
  }
#ifdef VDA_TS
  if (UPS && tid == 0 && blockIdx.x < 1024) {
    const unsigned long long rt = __builtin_amdgcn_s_memrealtime() - ts_rt0, cy = __builtin_amdgcn_s_memtime() - ts_c0;
    for (int c = 0; c < 10; ++c) { g_dts[blockIdx.x][c] = tsa[c]; g_dts[blockIdx.x][10 + c] = tsn[c]; }
    g_dts[blockIdx.x][20] = rt;
    g_dts[blockIdx.x][21] = cy;
    g_dts[blockIdx.x][22] = tsw;
  }
#endif
}

}  // namespace

#ifdef VDA_TS
extern "C" int vda_debug_oc1_timestamps(void* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dts), sizeof(g_dts), 0, hipMemcpyDeviceToHost);
}
#endif

// output_conv1 on the 2x resize of refinenet1's output without writing the resized map: the halo conv
// above with the resize fused into its patch staging (UPS).  x [BT, Hs, Ws, Cin] is the map BEFORE the
// bilinear (align_corners=True) resize to (H, W).  Returns 1 when the shape is not served.
int vda_conv_halo_fused(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int Hs, int Ws,
                        int H, int W, int Cin, int Cout, hipStream_t st, const float* bias9) {
  if (Cout != CO || Cin % CS != 0 || Hs > H || Ws > W || Hs < 1 || Ws < 1) return 1;
  if ((long)H * W * Cout * 2 >= (1L << 31)) return 1;  // the epilogue's per-frame buffer stores take 32-bit offsets
  if (!halo_fused_fits(Hs, Ws, H, W)) return 1;
  HaloGrid g;
  if (!halo_tile_grid(BT, H, W, DT, 1, 0x7fffffffL, g)) return vda_set_error(-22, "conv: too many tiles");
  // 4 interpolation waves (1 / 2: 2571 / 2080 vs 1801 us, profiles/r05_ab_oc1_interp_waves_dconv_separable.log)
  hipLaunchKernelGGL(halo_conv_kernel<true>, dim3(g.grid), dim3(768), 0, st, (const h16*)x, (const h16*)w, bias, (h16*)y,
                     relu, H, W, Cin, g.tiles_x, g.tiles_y, g.ntiles, Hs, Ws, bias9);
  VDA_LAUNCH_CHECK();
  return 0;
}

// the shapes vda_conv_halo_fused serves (no launch)
bool vda_conv_halo_fused_serves(int BT, int Hs, int Ws, int H, int W, int Cin, int Cout) {
  if (Cout != CO || Cin % CS != 0 || Hs > H || Ws > W || Hs < 1 || Ws < 1 || BT < 1) return false;
  if ((long)H * W * Cout * 2 >= (1L << 31) || !halo_fused_fits(Hs, Ws, H, W)) return false;
  HaloGrid g;
  return halo_tile_grid(BT, H, W, DT, 1, 0x7fffffffL, g);
}

// 3x3 / stride 1 / pad 1 conv, Cin % 64 == 0, Cout == 128, epilogue +bias [ReLU] (output_conv1,
// dpt.py:117, at 296^2): the halo tile cuts the 9x implicit-GEMM input re-read.  Returns 1 when the
// shape is not one this kernel serves (caller uses the implicit-GEMM conv).
int vda_conv_halo(const void* x, const void* w, void* y, const float* bias, int relu, int BT, int H, int W, int Cin,
                  int Cout, hipStream_t st) {
  if (Cout != CO || Cin % CS != 0) return 1;
  if ((long)H * W * Cout * 2 >= (1L << 31)) return 1;  // the epilogue's per-frame buffer stores take 32-bit offsets
  HaloGrid g;
  if (!halo_tile_grid(BT, H, W, DT, 1, 0x7fffffffL, g)) return vda_set_error(-22, "conv: too many tiles");
  hipLaunchKernelGGL(halo_conv_kernel<false>, dim3(g.grid), dim3(512), 0, st, (const h16*)x, (const h16*)w, bias,
                     (h16*)y, relu, H, W, Cin, g.tiles_x, g.tiles_y, g.ntiles, 0, 0);
  VDA_LAUNCH_CHECK();
  return 0;
}
