// Spatial (DINOv2) and temporal (motion-module) attention, fp16 MFMA + fp32 online softmax.
#include "vda_common.h"
#include "../../include/vda.h"
#include <type_traits>
#include <stdlib.h>

#ifdef VDA_TS  // per-block clock stamps of the spatial attention (tools/clock_probe.py; experiments only)
__device__ unsigned long long g_atsc[8192][4];
#define ATSC(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192) { \
    g_atsc[blockIdx.x][2 * (k)] = __builtin_amdgcn_s_memtime(); \
    g_atsc[blockIdx.x][2 * (k) + 1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
extern "C" int vda_debug_attn_clock_stamps(void* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_atsc), sizeof(g_atsc), 0, hipMemcpyDeviceToHost);
}
#else
#define ATSC(k) do {} while (0)
#endif

namespace {

// =============================================================================================
// Spatial attention, D = 64, v_mfma_f32_16x16x32_f16.  Block = 4 waves x 32 queries of one (batch,
// head); a wave owns two 16-query tiles qt, a lane query li = lane & 15 of each (qt adds 16) and the
// key / channel group g = lane >> 4.
//   Sᵀ[key][q] = K·Qᵀ   2 key tiles k2 x 2 query tiles x 2 K = 32 steps ks per 32-key half.  A = K row
//                       16 k2 + li, 16-byte chunk 4 ks + g (LDS, ds_read_b128), B = Q of query 16 qt + li
//                       (registers, pre-scaled by scale·log2e).  A chain starts from C = -m (4 registers of
//                       the query tile's running reference m, see the deferred re-base below), so the
//                       scores come out relative to it with no VALU subtraction.  Register r of tile
//                       (k2, qt) holds key 16 k2 + 4g + r.
//   Oᵀ += Vᵀ·Pᵀ         4 channel tiles ct x 2 query tiles, one K = 32 step per half.  B = P converted in
//                       place: {tile (0, qt), tile (1, qt)} is the lane's operand (k = 8g + j is key 4g + j
//                       for j < 4 and 16 + 4g + j - 4 above), no cross-lane move; A = Vᵀ in the same
//                       permuted key order by two ds_read_b64_tr_b16 (rows 4g + q4 and 16 below).  Register
//                       r of tile (ct, qt) holds channel 16 ct + 4g + r.
// Row state (m, the row sum, the re-base test) is per query tile; a lane's row sum covers its 8 keys of
// every half and is reduced across the four groups g once, in the epilogue.
// K/V tiles (64 keys x 64 channels, 8 KiB each) arrive by LDS-DMA (4 x 1-KiB pieces per wave per
// tile, keys >= N read as zeros) into a 2-slot ring, one barrier per tile.  The softmax unit is a
// 32-key half of the tile: its 8 QK MFMAs, 16 exponentials and 8 PV MFMAs, so only half a tile of
// scores / P is live: 120 VGPRs, FOUR waves per SIMD (4 blocks x 32 KiB of LDS per CU), which cover
// each other's LDS / MFMA / exp latency chains better than three waves of whole-tile work (152 VGPRs).
// Work the result does not need is left out: a wave whose 32 queries are all >= N (the last query
// block) only moves its DMA pieces and takes the barriers, and a half of the masked tail tile whose
// 32 keys are all >= N is skipped whole (it would add 0 to the row sum and 0 x 0 to O): 4.5 % of the
// wave x half units at N = 1370, 5.0 % at N = 2443.
// The two ring slots are two __shared__ objects and the tile loop is unrolled by 2 with static slots:
// with one ring array hipcc cannot prove that a tile's V reads do not alias the DMA in flight into the
// other slot and drains it (s_waitcnt vmcnt(0)) before every tile's first V read.  s_setprio 1 around
// the MFMA clusters lets a wave that reaches its MFMAs issue them ahead of the other waves' softmax VALU.
// The block -> (b, h, query block) map keeps all query blocks of one (b, h) on one XCD (K/V re-reads
// hit that L2).  LDS images: K slot row*8 + (chunk ^ ((row >> 1) & 7)), V slot row*8 + (chunk ^
// (((row >> 1) & 3) << 1)): conflict-free for the b128 K reads (16 rows of one chunk per 16 lanes) and
// the b64 transposed V reads (8 rows x 32 B per 32 lanes), checked by brute force over the lane groups.
// MFMA shape (profiles/attn_mfma16_ab.log, same box, random data, 32 x N x 16 heads): the 32x32x16 shape
// was chosen because its 32-cycle MFMA leaves 24 issue cycles per gap for the softmax VALU against 8
// for the 16-cycle 16x16x32.  With four waves per SIMD the other waves fill those gaps, and the chip
// holds a higher clock on 16x16x32.  Measured with the dead work skipped in both:
//   shape      N = 1370, us per call (median, min-max of 9 alternating rounds)   N = 2443     in-kernel clock (its own run)
//   parent     272.4 (271.9-273.6)   32x32x16, dead waves and halves computed     808.7        -
//   32x32x16   266.5 (265.2-267.4)                                                786.3        1.55 GHz
//   16x16x32   259.2 (258.8-261.1)   kept                                         769.5        1.75 GHz
// so skipping the dead work is worth 2.2 / 2.8 % and the shape another 2.7 / 2.1 % (fewer cycles per
// FLOP are not what it buys: at the clock each holds the 32x32x16 kernel is at 0.56 of the peak, this
// one at 0.52); smoke() rel-L1 7.89e-4 for both 32x32x16 builds, 6.77e-4 for this one (the K = 32 steps
// change the summation order; rel-L1 vs SDPA 4.70e-4 for all).  On top of it, the V fragments requested
// ahead of the softmax: 257.0 -> 254.8 us (N = 2443: 761.9 -> 759.2), bit-identical; the second half's K
// fragments requested ahead of the first half's PV MFMAs as well: no change (256.7 / 763.7), dropped.
// This kernel against the parent on a third box: 275.5 -> 253.8 us (-7.9 %), N = 2443 824.4 -> 756.7;
// bench.py 707.4 -> 714.0 frames/s, above the parent in each of 5 alternating pairs
// (profiles/attn_mfma16_forward_ab.log).
// Measured before (tools/ab_attn.py, same box, ViT-L 32 x 1370 x 16, 32x32x16): whole-tile softmax,
// 3-slot ring, three waves per SIMD (round 5) 292-298 us; halves at three waves per SIMD 297; halves +
// 4 waves/SIMD 282-289; + static slots 276; + s_setprio 272-275 (r06_ab_attn_*.log).  Rejected: 8-wave
// blocks (297-302), row sums by v_dot2 on the packed P (+3 %), the half's K reads issued ahead of the
// chain (no change), and a software-pipelined wave (the next half's QK chain issued under the current
// half's softmax, 3-slot ring, 2 / 3 waves per SIMD: 343 / 330 us, bit-identical:
// profiles/r06_ab_attn_pipe.log).  Earlier rounds: QK of tile t+1 before the softmax of tile t 333 vs
// 292 us; two 32-query sets per wave 317.8 / 307.8 vs 275.0 us (r05_ab_attn_two_sets.log).
// =============================================================================================
constexpr int SD = 64;       // head dim
constexpr int SA_KT = 64;    // keys per tile

// One A fragment of Vᵀ: two ds_read_b64_tr_b16.  Spatial kernel: the second read 16 key rows below the
// first (P's k order above).  Temporal kernels (32x32x16 layouts, lane r32 = lane & 31, hf = lane >> 5
// owns query r32): 8 rows below (P's k order 8(j>>2) + 4hf + (j&3) within a 16-key slice).
__device__ __forceinline__ h8 vt_frag(const h16* p0, const h16* p1) {
  const h4 v0 = lds_read_tr16(p0), v1 = lds_read_tr16(p1);
  return h8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
}
// Temporal kernels: an Oᵀ tile dt holds query r32's channels d = dt*32 + 8gq + 4hf .. + 3 in registers
// 4gq .. 4gq + 3: the first channel of group gq, and the group normalised by inv = 1 / row sum as fp16.
__device__ __forceinline__ int o_chan(int dt, int gq, int hf) { return dt * 32 + 8 * gq + 4 * hf; }
__device__ __forceinline__ h4 o_group(const f16x& o, int gq, float inv) {
  h4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (h16)(o[gq * 4 + r] * inv);
  return v;
}

__device__ __forceinline__ int sa_kslot(int row, int c) { return row * 8 + (c ^ ((row >> 1) & 7)); }
__device__ __forceinline__ int sa_vslot(int row, int c) { return row * 8 + (c ^ (((row >> 1) & 3) << 1)); }
// max / sum over the four 16-lane groups (lanes l, l ^ 16, l ^ 32, l ^ 48)
__device__ __forceinline__ float quad_max(float v) { float a, b; swap16_pair(v, a, b); return half_max(fmaxf(a, b)); }
__device__ __forceinline__ float quad_sum(float v) { float a, b; swap16_pair(v, a, b); return half_sum(a + b); }
__global__ __launch_bounds__(256, 4) void spatial_attn16_kernel(const h16* __restrict__ qkv, h16* __restrict__ out,
                                                                int N, int H, int nqb, int nblocks, float scale_log2) {
  __shared__ __attribute__((aligned(16))) h16 sKV0[2][SA_KT * SD];  // ring slot 0: [K | V]
  __shared__ __attribute__((aligned(16))) h16 sKV1[2][SA_KT * SD];  // ring slot 1
  ATSC(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int id = blockIdx.x;
  const int per = nblocks >> 3;
  if (id < per * 8) id = (id & 7) * per + (id >> 3);
  const int qb = __builtin_amdgcn_readfirstlane(id % nqb), bh = id / nqb;  // scalar (the buffer
  const int h = __builtin_amdgcn_readfirstlane(bh % H), b = __builtin_amdgcn_readfirstlane(bh / H);  // rsrc)
  const int C = H * SD;
  const long ld = 3L * C;
  const h16* base = qkv + (long)b * N * ld + h * SD;
  const int li = lane & 15, g = lane >> 4, q4 = li >> 2, p4 = li & 3;
  const int q0 = qb * 128 + wave * 32 + li;  // query of tile 0; tile 1 is q0 + 16
  // A wave whose 32 queries are all >= N only moves its DMA pieces and takes the barriers: no Q load,
  // QK, softmax, PV or store (wave-uniform).
  const bool live = qb * 128 + wave * 32 < N;

  h8 qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      h8 t = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (q0 + 16 * qt < N) t = __builtin_bit_cast(h8, ldg16(base + (long)(q0 + 16 * qt) * ld + ks * 32 + g * 8));
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = (h16)((float)t[e] * scale_log2);
      qf[qt][ks] = t;
    }

  // 16 pieces per tile (8 K + 8 V, 8 key rows each); wave w moves pieces 4w .. 4w+3.  Buffer loads
  // with the (b, h) rows as the record range: keys >= N read as zeros.  Per-lane offsets are fixed
  // across tiles (the tile advances by the scalar offset).
  const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)((long)N * ld * 2), 0x00020000);
  unsigned voff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gp = wave * 4 + j, isv = gp >> 3, pc = gp & 7;
    const int slot = pc * 64 + lane, row = slot >> 3, pos = slot & 7;
    const int c = isv ? (pos ^ (((row >> 1) & 3) << 1)) : (pos ^ ((row >> 1) & 7));
    voff[j] = (unsigned)(((long)row * ld + (isv ? 2 * C : C) + c * 8) * 2);
  }
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  // slot as a compile-time constant (the unrolled loop) or a run-time int (the tiles outside it)
  auto slot_ptr = [&](auto sl, int isv) -> h16* {
    if constexpr (std::is_same<decltype(sl), int>::value) return sl ? sKV1[isv] : sKV0[isv];
    else return decltype(sl)::value == 0 ? sKV0[isv] : sKV1[isv];
  };
  auto dma = [&](int kt, auto sl) {  // tile kt -> ring slot sl (= kt & 1)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gp = wave * 4 + j, isv = gp >> 3, pc = gp & 7;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (VDA_LDS void*)(slot_ptr(sl, isv) + pc * 512), 16, (int)voff[j],
                                               (int)(kt * SA_KT * ld * 2), 0, 0);
    }
  };

  f4 o[4][2];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) o[ct][0] = o[ct][1] = f4{0.f, 0.f, 0.f, 0.f};
  f4 negm[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
  float mrun[2] = {0.f, 0.f}, lsum[2] = {0.f, 0.f};

  // Lane-constant LDS byte offsets: K fragment ks of key row li (key tile k2 adds 16 rows = 2 KiB, key
  // block kb 32 rows = 4 KiB); transposed-V read base of channel tile ct (the second read of a fragment
  // adds 16 rows = 2 KiB; the swizzle terms repeat every 16 / 8 rows).
  unsigned kofs[2], vofs[4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) kofs[ks] = (unsigned)sa_kslot(li, ks * 4 + g) * 16u;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int col = ct * 16 + 4 * p4, r0 = 4 * g + q4;
    vofs[ct] = (unsigned)(sa_vslot(r0, col >> 3) * 8 + (col & 7)) * 2u;
  }
  // Deferred re-base (FA-style online softmax without a per-tile max): P = exp2(S - m) against the
  // running reference m; a half only re-bases when a lane's P sum passes 2^15 (then some P may not fit
  // fp16: the scores are recomputed, the true max taken and the half redone), so the steady state
  // computes no max at all.  P <= 2^15 keeps P exact to fp16 rounding and the fp32 sums far from
  // overflow.  The first half of the first tile always re-bases (m starts at 0, not at a real max).
  auto tile = [&](int kt, auto first_tag, auto mask_tag, auto sl) {
    constexpr bool FIRST = decltype(first_tag)::value;
    constexpr bool MASK = decltype(mask_tag)::value;
    if (!live) return;
    const char* kbase = reinterpret_cast<const char*>(slot_ptr(sl, 0));
    const char* vbase = reinterpret_cast<const char*>(slot_ptr(sl, 1));
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      // A half of the tail tile whose 32 keys are all >= N (scalar; only kb == 1 can meet it, the tile's
      // first key is real) would add tt = 0 to lsum and 0 x 0 to o: skipped whole.
      if (MASK && kt * SA_KT + kb * 32 >= N) continue;
      f4 s1[2][2];  // [key tile][query tile]
      auto qk = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) {
            const h8 kf = *reinterpret_cast<const h8*>(kbase + kofs[ks] + kb * 4096 + k2 * 2048);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) s1[k2][qt] = mfma16(kf, qf[qt][ks], ks == 0 ? negm[qt] : s1[k2][qt]);
          }
        if constexpr (MASK) {
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (kt * SA_KT + kb * 32 + 16 * k2 + 4 * g + r >= N) s1[k2][0][r] = s1[k2][1][r] = -INFINITY;
        }
      };
      auto smax = [&](int qt) {
        const f4 a = s1[0][qt], c = s1[1][qt];
        float mx = fmaxf(fmaxf(a[0], a[1]), a[2]);
        mx = fmaxf(fmaxf(mx, a[3]), c[0]);
        mx = fmaxf(fmaxf(mx, c[1]), c[2]);
        return quad_max(fmaxf(mx, c[3]));
      };
      auto rebase = [&](int qt, float sh) {
        mrun[qt] += sh;
#pragma unroll
        for (int r = 0; r < 4; ++r) negm[qt][r] = -mrun[qt];
        s1[0][qt] -= sh;
        s1[1][qt] -= sh;
      };
      h8 pf[2];
      float tt[2];
      auto expo = [&]() {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const float pv = __builtin_amdgcn_exp2f(s1[r >> 2][qt][r & 3]);
            tt[qt] = r == 0 ? pv : tt[qt] + pv;
            pf[qt][r] = (h16)pv;
          }
      };
      __builtin_amdgcn_s_setprio(1);
      qk();
      __builtin_amdgcn_s_setprio(0);
      // the half's four Vᵀ fragments requested here, so their LDS latency passes under the softmax VALU
      // (left to the scheduler they are issued in front of the PV MFMAs that wait for them)
      h8 vf[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const h16* va = reinterpret_cast<const h16*>(vbase + vofs[ct] + kb * 4096);
        vf[ct] = vt_frag(va, va + 16 * SD);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (FIRST && kb == 0) {
        rebase(0, smax(0));
        rebase(1, smax(1));
        expo();
      } else {
        expo();
        if (__any(!(fmaxf(tt[0], tt[1]) <= 32768.f))) {  // rare: re-base this half on its true max and redo it
          qk();  // the scores again (the K slot is still resident): they need not stay live past expo
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) {
            const float sh = fmaxf(smax(qt), 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-sh);
            lsum[qt] *= alpha;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) o[ct][qt] *= alpha;
            rebase(qt, sh);
          }
          expo();
        }
      }
      lsum[0] += tt[0];
      lsum[1] += tt[1];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {  // 8 independent MFMAs, a V fragment feeds both query tiles
        o[ct][0] = mfma16(vf[ct], pf[0], o[ct][0]);
        o[ct][1] = mfma16(vf[ct], pf[1], o[ct][1]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  };
  const int ntiles = (N + SA_KT - 1) / SA_KT;
  // tile kt landed and visible (its DMA is this wave's only one in flight), and every wave is done with
  // tile kt - 1: its slot takes tile kt + 1
  auto enter = [&](int kt, auto next_slot) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as the builtin: hipcc's own wait bookkeeping sees it
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");  // compiler-only: no LDS read of tile kt moves above the barrier
    if (kt + 1 < ntiles) dma(kt + 1, next_slot);
  };
  // a tile whose slot is only known at run time (the first, an odd leftover and the partial last one)
  auto tile_any = [&](int kt, auto first_tag, auto mask_tag) {
    enter(kt, (kt + 1) & 1);
    tile(kt, first_tag, mask_tag, kt & 1);
  };
  dma(0, S0{});
  const bool tail = N % SA_KT != 0;
  if (ntiles == 1 && tail) tile_any(0, std::true_type{}, std::true_type{});
  else tile_any(0, std::true_type{}, std::false_type{});
  const int nfull = ntiles - (tail ? 1 : 0);
  int kt = 1;
  for (; kt + 1 < nfull; kt += 2) {  // pairs: odd kt in slot 1, even kt + 1 in slot 0
    enter(kt, S0{});
    tile(kt, std::false_type{}, std::false_type{}, S1{});
    enter(kt + 1, S1{});
    tile(kt + 1, std::false_type{}, std::false_type{}, S0{});
  }
  if (kt < nfull) tile_any(kt, std::false_type{}, std::false_type{});
  if (tail && ntiles > 1) tile_any(ntiles - 1, std::false_type{}, std::true_type{});
  // epilogue: the row sums across the four key groups, then channels 16 ct + 4g .. + 3 of each query
  if (live) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float inv = 1.f / quad_sum(lsum[qt]);
      const int q = q0 + 16 * qt;
      if (q < N) {
        h16* op = out + ((long)b * N + q) * C + h * SD + 4 * g;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          h4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (h16)(o[ct][qt][r] * inv);
          *reinterpret_cast<h4*>(op + ct * 16) = v;
        }
      }
    }
  }
  ATSC(1);
}

// =============================================================================================
// Temporal attention: one wave per (batch, site s, head), T <= 32 frames, v_mfma_f32_32x32x16_f16.
//   Sᵀ[key][q] = Σ_d K[key][d] Q[q][d]       A = K rows, B = Q rows (fragments straight from HBM)
//   Oᵀ[d][q]   = Σ_key Vᵀ[d][key] Pᵀ[key][q]  B = Pᵀ accumulator registers 8s..8s+7 (k order
//                16s + 8(j>>2) + 4h + (j&3)), A = Vᵀ by ds_read_b64_tr_b16 from a per-wave V tile.
// DP = head dim padded to a multiple of 16 (zero-filled, <= 192), NDT = 32-wide output d tiles.
// =============================================================================================
// pe='rope' (attention.py:403-429): rotate the 4 channel pairs of an 8-channel q and k fragment of
// frame t, first channel c0 (even) of C: angle t * theta^(-2i/C) for pair i, fp32 math on the fp16
// values (the reference's q.float() complex multiply, type_as back to fp16)
// (cos, sin) of frame t's angle for pair i.  Deliberately a real function: one copy of the powf / sincosf
// code in the file instead of one per unrolled site (4x the kernel's code otherwise), no out-pointers
// and so no scratch, and the RoPE outputs keep their bits: with the math inlined into the kernels some
// outputs moved in the last place (profiles/attn_selfcontained_bit_identity.log).
__device__ __noinline__ float2 rope_cs(int t, int i, int C, float theta) {
  const float freq = 1.f / powf(theta, (float)(2 * i) / (float)C);
  float sn, cs;
  sincosf((float)t * freq, &sn, &cs);
  return make_float2(cs, sn);
}
__device__ __forceinline__ void rope_frag(h8& q, h8& k, int t, int c0, int C, float theta) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float2 r = rope_cs(t, (c0 >> 1) + j, C, theta);
    const float cs = r.x, sn = r.y;
    const float qa = (float)q[2 * j], qb = (float)q[2 * j + 1];
    const float ka = (float)k[2 * j], kb = (float)k[2 * j + 1];
    q[2 * j] = (h16)(qa * cs - qb * sn);
    q[2 * j + 1] = (h16)(qa * sn + qb * cs);
    k[2 * j] = (h16)(ka * cs - kb * sn);
    k[2 * j + 1] = (h16)(ka * sn + kb * cs);
  }
}

__device__ __attribute__((aligned(64))) uint4 g_ta_zero[4];

// ---- the stages both temporal kernels share: they differ in how a K / Q fragment and the V tile
// are fetched and in how an output tile is stored ----
// work item -> (batch b, site s, head hh), heads fastest
__device__ __forceinline__ void ta_item(long item, int S, int H, int& b, int& s, int& hh) {
  hh = (int)(item % H);
  const long bs = item / H;
  s = (int)(bs % S);
  b = (int)(bs / S);
}
// Base-2 softmax of query r32 over the 32 keys of Sᵀ (the lane holds keys (r&3) + 8(r>>2) + 4hf, its
// partner lane ^ 32 the rest; keys >= T are masked): P as the two B fragments of the PV MFMAs;
// returns 1 / row sum.
__device__ __forceinline__ float ta_softmax(f16x acc, int T, int hf, float scale_log2, h8 (&pf)[2]) {
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int key = (r & 3) + 8 * (r >> 2) + 4 * hf;
    float t = acc[r] * scale_log2;
    if (key >= T) t = -INFINITY;
    acc[r] = t;
    mx = fmaxf(mx, t);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float p = exp2f(acc[r] - mx);
    sum += p;
    pf[r >> 3][r & 7] = (h16)p;
  }
  sum += __shfl_xor(sum, 32, 64);
  return 1.f / sum;
}
// Where a lane's tr16 reads of the row-major V tile start for output tile dt, key slice st: 16-lane
// group grp covers key rows 16st + 4(grp>>1) + q4 (and + 8), columns dt*32 + (grp&1)*16 + 4p4
__device__ __forceinline__ void ta_vpos(int lane, int dt, int st, int& r0, int& col) {
  const int grp = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  r0 = 16 * st + 4 * (grp >> 1) + q4;
  col = dt * 32 + (grp & 1) * 16 + 4 * p4;
}

constexpr int VDA_TA_NW = 4;  // waves (heads of one site) per temporal-attention block
template <int DP>
__global__ __launch_bounds__(64 * VDA_TA_NW) void temporal_attn_kernel(const h16* __restrict__ qkv, h16* __restrict__ out,
                                                            int B, int T, int S, int H, int D, float scale_log2,
                                                            float rope_theta) {
  constexpr int NST = DP / 16;
  constexpr int NDT = (DP + 31) / 32;
  constexpr int DP32 = NDT * 32;
  constexpr int VSTR = DP32 + (DP32 > 32 ? 32 : 0);  // row stride (halfs) of the V tile
  __shared__ __attribute__((aligned(16))) h16 sV[VDA_TA_NW][32 * VSTR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long item = (long)blockIdx.x * VDA_TA_NW + wave;
  const bool active = item < (long)B * S * H;  // the last block's waves past the last item idle as item 0
  int b, s, hh;
  ta_item(active ? item : 0, S, H, b, s, hh);
  const int C = H * D;
  const long ld = 3L * C;
  const int r32 = lane & 31, hf = lane >> 5;
  h16* vt = sV[wave];

  // V tile -> LDS (rows = keys, zero beyond T / D)
  {
    constexpr int CPR = DP32 / 8;  // 16-B chunks per row
    for (int i = lane; i < 32 * CPR; i += 64) {
      const int key = i / CPR, ch = i - key * CPR;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (active && key < T && ch * 8 < D)
        v = ldg16(qkv + ((long)(b * T + key) * S + s) * ld + 2 * C + hh * D + ch * 8);
      *reinterpret_cast<uint4*>(vt + key * VSTR + ch * 8) = v;
    }
  }
  // Sᵀ
  f16x acc = {};
  const long krow = ((long)(b * T + r32) * S + s) * ld + hh * D;
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const int d0 = st * 16 + hf * 8;
    h8 kf = h8{0, 0, 0, 0, 0, 0, 0, 0}, qf = kf;
    if (active && r32 < T && d0 < D) {
      qf = __builtin_bit_cast(h8, ldg16(qkv + krow + d0));
      kf = __builtin_bit_cast(h8, ldg16(qkv + krow + C + d0));
      if (rope_theta > 0.f) rope_frag(qf, kf, r32, hh * D + d0, C, rope_theta);
    }
    acc = mfma32(kf, qf, acc);
  }
  h8 pf[2];
  const float inv = ta_softmax(acc, T, hf, scale_log2, pf);
  __syncthreads();  // V tile visible to the whole wave (all waves reach this)

#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    f16x o = {};
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      int r0, col;
      ta_vpos(lane, dt, st, r0, col);
      o = mfma32(vt_frag(vt + r0 * VSTR + col, vt + (r0 + 8) * VSTR + col), pf[st], o);
    }
    if (active && r32 < T) {
      h16* op = out + ((long)(b * T + r32) * S + s) * C + hh * D;
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = o_chan(dt, gq, hf);
        if (d < D) *reinterpret_cast<h4*>(op + d) = o_group(o, gq, inv);
      }
    }
  }
}

// Temporal attention with the (site, head)'s q, k and v rows staged in LDS (north_star; verdict r1
// item 10).  The direct-load kernel above reads its K / Q fragments as 32-B pieces of 32 different
// frame rows per instruction (rows S * 3C apart), which held it at ~3.5 TB/s.  Here each wave moves
// its head's three 32 x D tiles into LDS with global_load_lds, 16 B per lane, whole D*2-B row
// segments per 16 / 4 / 2 lanes (D = 128 / 64 / 32), then reads the MFMA fragments from LDS.  LDS
// image: row r of a tile = D halfs, 16-B chunk c at position c ^ ((r / (16 / CH)) & (CH - 1)),
// CH = D / 8: conflict-free for the K / Q fragment reads (ds_read_b128 lane groups = 16 rows of one
// chunk).  The output goes back through the q tile so it is stored as whole row segments too.
// Waves never share LDS, so the only sync is each wave's own vmcnt + one block barrier.
// Invariant: H % NW == 0 (vda_temporal_attention launches this kernel for no other H), so B * S * H
// is a multiple of NW, the grid has exactly B * S * H / NW blocks and every wave has an item.
template <int D, int NW>
__global__ __launch_bounds__(64 * NW) void temporal_attn_lds_kernel(const h16* __restrict__ qkv, h16* __restrict__ out,
                                                                  int T, int S, int H, float scale_log2,
                                                                  float rope_theta) {
  constexpr int CH = D / 8;                 // 16-B chunks per row
  constexpr int RPG = 16 / CH;              // rows per 256-B bank line
  constexpr int TILE = 32 * D;              // halfs per tensor tile
  constexpr int NI = 32 * CH / 64;          // DMA instructions per tensor
  constexpr int NST = D / 16;
  constexpr int NDT = D / 32;
  __shared__ __attribute__((aligned(16))) h16 sm[NW * 3 * TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b, s, hh;
  ta_item((long)blockIdx.x * NW + wave, S, H, b, s, hh);
  const int C = H * D;
  const long ld = 3L * C;
  h16* tq = sm + wave * 3 * TILE;
  h16* tk = tq + TILE;
  h16* tv = tk + TILE;
  auto pos = [](int row, int c) { return c ^ ((row / RPG) & (CH - 1)); };

  // stage q, k, v: slot sl = i * 64 + lane of a tile holds row sl / CH, chunk pos(row, sl % CH)
#pragma unroll
  for (int z = 0; z < 3; ++z) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int sl = i * 64 + lane;
      const int row = sl / CH;
      const int c = pos(row, sl % CH);
      const void* src = g_ta_zero;
      if (row < T) src = qkv + ((long)(b * T + row) * S + s) * ld + z * C + hh * D + c * 8;
      __builtin_amdgcn_global_load_lds(src, (VDA_LDS void*)(tq + z * TILE + i * 512), 16, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // Sᵀ = K Qᵀ: lane (r32, hf) holds K / Q row r32, channels st * 16 + hf * 8 .. + 7; rows >= T are
  // zero in LDS and masked in the softmax
  const int r32 = lane & 31, hf = lane >> 5;
  f16x acc = {};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const int c = st * 2 + hf;
    h8 kf = *reinterpret_cast<const h8*>(tk + r32 * D + pos(r32, c) * 8);
    h8 qf = *reinterpret_cast<const h8*>(tq + r32 * D + pos(r32, c) * 8);
    if (rope_theta > 0.f) rope_frag(qf, kf, r32, hh * D + c * 8, C, rope_theta);
    acc = mfma32(kf, qf, acc);
  }
  h8 pf[2];
  const float inv = ta_softmax(acc, T, hf, scale_log2, pf);

#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    f16x o = {};
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      int r0, col;
      ta_vpos(lane, dt, st, r0, col);
      o = mfma32(vt_frag(tv + r0 * D + pos(r0, col >> 3) * 8 + (col & 7),
                         tv + (r0 + 8) * D + pos(r0 + 8, col >> 3) * 8 + (col & 7)), pf[st], o);
    }
    // into the q tile (its fragments are consumed) as rows, so the stores below write whole D*2-B
    // row segments
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int d = o_chan(dt, gq, hf);
      *reinterpret_cast<h4*>(tq + r32 * D + pos(r32, d >> 3) * 8 + (d & 7)) = o_group(o, gq, inv);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int sl = i * 64 + lane;
    const int row = sl / CH, c = sl % CH;
    const uint4 v = *reinterpret_cast<const uint4*>(tq + row * D + pos(row, c) * 8);
    if (row < T) *reinterpret_cast<uint4*>(out + ((long)(b * T + row) * S + s) * C + hh * D + c * 8) = v;
  }
}

// The staged kernel for D = 192 (ViT-g's motion modules 0 / 1: C = 1536, 8 heads).  A row is 24 16-B chunks, no
// power of two, so the XOR swizzle above does not apply: rows are padded instead, each tile to the stride its
// reads want (tools/ta192_stride.py tries every stride against the LDS bank rules):
//   q, k tiles: 25 chunks (400 B).  A ds_read_b128 lane group is 16 rows of one chunk, rows {0-3, 12-15, 20-27}
//               (+4, +32): every residue mod 16 once, and an odd stride permutes them over the 16 slots of the
//               256-B bank row: conflict-free.
//   v tile:     28 chunks (448 B), the direct kernel's VSTR: a 32-lane group of ds_read_b64_tr_b16 reads 64 B
//               of 4 consecutive rows, and 448 = 192 (mod 256) lays the four pieces side by side.
// global_load_lds fills a tile lane-linearly, 64 chunks per instruction, so slot sl is row sl / CS, chunk
// sl % CS of the padded image; the pad chunks and the rows >= T read the zero page.  13 instructions (12.5
// used) per q / k tile, 14 per v tile: 13 + 13 + 14 KiB = 40 KiB of LDS per wave for the three tiles (36 KiB
// of it data), 80 KiB per 2-wave block, two blocks per CU.  The output leaves through the q tile as whole
// 384-B row segments.  Invariant as above: H % NW == 0.
template <int NW>
__global__ __launch_bounds__(64 * NW) void temporal_attn_lds192_kernel(const h16* __restrict__ qkv, h16* __restrict__ out,
                                                                      int T, int S, int H, float scale_log2,
                                                                      float rope_theta) {
  constexpr int D = 192, CH = D / 8;
  constexpr int CQ = 25, CV = 28;             // chunks per padded row
  constexpr int SQ = CQ * 8, SV = CV * 8;     // row strides (halfs)
  constexpr int NIQ = (32 * CQ + 63) / 64, NIV = (32 * CV + 63) / 64;  // DMA instructions per tile
  constexpr int TQ = NIQ * 512, TV = NIV * 512;                        // halfs per tile: whole instructions
  constexpr int NST = D / 16, NDT = D / 32;
  __shared__ __attribute__((aligned(16))) h16 sm[NW * (2 * TQ + TV)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b, s, hh;
  ta_item((long)blockIdx.x * NW + wave, S, H, b, s, hh);
  const int C = H * D;
  const long ld = 3L * C;
  h16* tq = sm + wave * (2 * TQ + TV);
  h16* tk = tq + TQ;
  h16* tv = tk + TQ;

#pragma unroll
  for (int z = 0; z < 3; ++z) {
    const int cs = z < 2 ? CQ : CV, ni = z < 2 ? NIQ : NIV;
    h16* base = z == 0 ? tq : z == 1 ? tk : tv;
#pragma unroll
    for (int i = 0; i < NIV; ++i) {
      if (i < ni) {
        const int sl = i * 64 + lane;
        const int row = sl / cs, c = sl - row * cs;
        const void* src = g_ta_zero;
        if (row < T && c < CH) src = qkv + ((long)(b * T + row) * S + s) * ld + z * C + hh * D + c * 8;
        __builtin_amdgcn_global_load_lds(src, (VDA_LDS void*)(base + i * 512), 16, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int r32 = lane & 31, hf = lane >> 5;
  f16x acc = {};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const int c = st * 2 + hf;
    h8 kf = *reinterpret_cast<const h8*>(tk + r32 * SQ + c * 8);
    h8 qf = *reinterpret_cast<const h8*>(tq + r32 * SQ + c * 8);
    if (rope_theta > 0.f) rope_frag(qf, kf, r32, hh * D + c * 8, C, rope_theta);
    acc = mfma32(kf, qf, acc);
  }
  h8 pf[2];
  const float inv = ta_softmax(acc, T, hf, scale_log2, pf);

#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    f16x o = {};
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      int r0, col;
      ta_vpos(lane, dt, st, r0, col);
      o = mfma32(vt_frag(tv + r0 * SV + col, tv + (r0 + 8) * SV + col), pf[st], o);
    }
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {  // into the q tile (its fragments are consumed), as rows
      const int d = o_chan(dt, gq, hf);
      *reinterpret_cast<h4*>(tq + r32 * SQ + d) = o_group(o, gq, inv);
    }
  }
  __builtin_amdgcn_wave_barrier();  // the row reads below follow the other lanes' writes (one wave: LDS is in order)
#pragma unroll
  for (int i = 0; i < 32 * CH / 64; ++i) {
    const int sl = i * 64 + lane;
    const int row = sl / CH, c = sl - row * CH;
    const uint4 v = *reinterpret_cast<const uint4*>(tq + row * SQ + c * 8);
    if (row < T) *reinterpret_cast<uint4*>(out + ((long)(b * T + row) * S + s) * C + hh * D + c * 8) = v;
  }
}

// vda_debug_attn (tuning build): 1 = the direct-load temporal kernel for every head dim
VDA_KNOB(int, g_ta_direct, 0);

}  // namespace

#ifdef VDA_TUNING
extern "C" int vda_debug_attn(int32_t temporal_direct) {
  g_ta_direct = temporal_direct;
  return 0;
}
#endif

extern "C" int vda_spatial_attention(const void* qkv, void* out, int32_t B, int32_t N, int32_t H,
                                     int32_t D, float scale, void* stream) {
  VDA_CHECK_ARG(qkv && out, "null pointer");
  VDA_CHECK_ARG(B > 0 && N > 0 && H > 0, "empty attention");
  VDA_CHECK_ARG(D == SD, "spatial attention supports head dim 64 only");
  const int nqb = (N + 127) / 128;
  const long nb = (long)nqb * H * B;
  VDA_CHECK_ARG(nb < 0x7fffffffL, "attention grid too large");
  hipLaunchKernelGGL(spatial_attn16_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const h16*)qkv,
                     (h16*)out, N, H, nqb, (int)nb, scale * 1.4426950408889634f);
  VDA_LAUNCH_CHECK();
  return 0;
}

extern "C" int vda_temporal_attention(const void* qkv, void* out, int32_t B, int32_t T, int32_t S,
                                      int32_t H, int32_t D, float scale, float rope_theta, void* stream) {
  VDA_CHECK_ARG(qkv && out, "null pointer");
  VDA_CHECK_ARG(B > 0 && S > 0 && H > 0, "empty attention");
  VDA_CHECK_ARG(T > 0 && T <= 32, "temporal attention needs 1 <= T <= 32 (PE table length)");
  VDA_CHECK_ARG(D > 0 && D % 8 == 0 && D <= 192, "head dim must be a multiple of 8, <= 192");
  const long items = (long)B * S * H;
  dim3 grid((unsigned)((items + VDA_TA_NW - 1) / VDA_TA_NW));
  hipStream_t st = (hipStream_t)stream;
  const float sl = scale * 1.4426950408889634f;
  // q / k / v rows staged in LDS for the head dims the model uses (128 at C = 1024, 32 at C = 256, 8
  // heads); the direct-load kernel below serves the other head dims (every D % 8 == 0 up to 192)
  if (!g_ta_direct && (D == 32 || D == 64 || D == 128)) {
    const int nw = D == 128 ? 2 : 4;  // 24 / 12 / 6 KiB of LDS per wave
    if (H % nw == 0) {  // the LDS kernel's invariant: no idle wave
      const unsigned g = (unsigned)(items / nw);
      if (D == 128)
        hipLaunchKernelGGL((temporal_attn_lds_kernel<128, 2>), dim3(g), dim3(128), 0, st, (const h16*)qkv, (h16*)out, T,
                           S, H, sl, rope_theta);
      else if (D == 64)
        hipLaunchKernelGGL((temporal_attn_lds_kernel<64, 4>), dim3(g), dim3(256), 0, st, (const h16*)qkv, (h16*)out, T,
                           S, H, sl, rope_theta);
      else
        hipLaunchKernelGGL((temporal_attn_lds_kernel<32, 4>), dim3(g), dim3(256), 0, st, (const h16*)qkv, (h16*)out, T,
                           S, H, sl, rope_theta);
      VDA_LAUNCH_CHECK();
      return 0;
    }
  }
  // D = 192 (ViT-g's C = 1536): staged too, by measurement (32 x 1,369 sites, 8 heads: 118.7 us = 4.5 TB/s against
  // the direct-load kernel's 171.0, profiles/vitg_temporal_d192.log); 40 KiB of LDS per wave, 2 waves per block
  if (!g_ta_direct && D == 192 && H % 2 == 0) {
    hipLaunchKernelGGL((temporal_attn_lds192_kernel<2>), dim3((unsigned)(items / 2)), dim3(128), 0, st, (const h16*)qkv,
                       (h16*)out, T, S, H, sl, rope_theta);
    VDA_LAUNCH_CHECK();
    return 0;
  }
  const int dp = (D + 15) / 16 * 16;
#define VDA_TA(DPV) hipLaunchKernelGGL(temporal_attn_kernel<DPV>, grid, dim3(64 * VDA_TA_NW), 0, st, (const h16*)qkv, (h16*)out, B, T, S, H, D, sl, rope_theta)
  switch (dp) {
    case 16: VDA_TA(16); break;
    case 32: VDA_TA(32); break;
    case 48: VDA_TA(48); break;
    case 64: VDA_TA(64); break;
    case 80: VDA_TA(80); break;
    case 96: VDA_TA(96); break;
    case 112: VDA_TA(112); break;
    case 128: VDA_TA(128); break;
    // D 136 .. 192 (ViT-g's motion modules 0 / 1: C = 1536, 8 heads): the V tile is 4 x 32 x 224 halfs = 56 KiB
    case 144: VDA_TA(144); break;
    case 160: VDA_TA(160); break;
    case 176: VDA_TA(176); break;
    default: VDA_TA(192); break;
  }
#undef VDA_TA
  VDA_LAUNCH_CHECK();
  return 0;
}
