// One-tile-per-block MFMA GEMM / implicit-GEMM conv kernels: the X-tile loaders, the shared epilogues
// (epi_store4, epi_geglu4), gemm_reg_kernel and gemm_kernel.  Device code of vda_gemm.hip, which is its
// only includer: the launch logic and the set of instantiations live there.
//
// Both kernels issue the MFMA in the "swapped" orientation: the A operand is a 16-row slice of W (output
// channels) and the B operand a 16-row slice of X (tokens/pixels), so each lane ends up holding FOUR
// CONSECUTIVE OUTPUT CHANNELS of one token: the epilogue does 8-byte loads/stores of bias/residual/output
// and the GEGLU pair (h, g) of a channel lands in the same lane.
//
// gemm_reg_kernel: BM x BN block tile, BK = 64, 256 threads = 4 waves as 2 (m) x 2 (n), register-staged
// double-buffered LDS (global loads for tile t+1 are issued before the MFMAs of tile t, written to the
// other LDS buffer after them; one barrier per K tile).  LDS rows are 128 B (64 halfs) with the 16-B chunk
// index XOR-swizzled by (row>>1)&7, which makes both the ds_write_b128 stores and the 16-lane
// ds_read_b128 fragment reads bank-conflict free.  gemm_kernel: see its own comment below.
#pragma once
#include "vda_internal.h"
#include "vda_halo.h"

namespace {

constexpr int BK = 64;

__device__ __forceinline__ int swz(int row, int chunk) {  // half offset in a [rows][64] tile
  return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3);
}

// ---- X-tile loaders -------------------------------------------------------------------------
// Dense: X is a row-major [M, K] matrix with row stride ldx.
struct DenseLoader {
  const h16* rowp[4];
  bool rowok[4];
  __device__ void init(const GemmParams& p, int m0, int tid, int nrow_iters) {
    for (int i = 0; i < nrow_iters; ++i) {
      int r = (tid >> 3) + 32 * i;
      int m = m0 + r;
      rowok[i] = m < p.M;
      rowp[i] = p.x + (long)(rowok[i] ? m : 0) * p.ldx;
    }
  }
  __device__ uint4 load(const GemmParams& p, int i, int k) const {
    if (rowok[i] && k < p.K) return ldg16(rowp[i] + k);
    return make_uint4(0, 0, 0, 0);
  }
};

// Implicit GEMM conv: row m = output pixel (bt, oy, ox), k = (ky*ks + kx)*Cin + ci.
struct ConvLoader {
  int bt[4], oy[4], ox[4];
  bool rowok[4];
  __device__ void init(const GemmParams& p, int m0, int tid, int nrow_iters) {
    for (int i = 0; i < nrow_iters; ++i) {
      int r = (tid >> 3) + 32 * i;
      int m = m0 + r;
      rowok[i] = m < p.M;
      int mm = rowok[i] ? m : 0;
      ox[i] = mm % p.Wo;
      int t = mm / p.Wo;
      oy[i] = t % p.Ho;
      bt[i] = t / p.Ho;
    }
  }
  __device__ uint4 load(const GemmParams& p, int i, int k) const {
    if (!rowok[i] || k >= p.K) return make_uint4(0, 0, 0, 0);
    int tap = k / p.Cin;
    int ci = k - tap * p.Cin;
    int ky = tap / p.ks, kx = tap - ky * p.ks;
    int iy = oy[i] * p.stride - p.pad + ky;
    int ix = ox[i] * p.stride - p.pad + kx;
    uint4 v;
    if (p.up_h > 0) {
      // conv input = bilinear(align_corners=True) upsample of the stored [H, W] map to [up_h, up_w]
      if (iy < 0 || iy >= p.up_h || ix < 0 || ix >= p.up_w) return make_uint4(0, 0, 0, 0);
      int y0, y1, x0, x1;
      float wy, wx;
      ac_coord(iy, p.H, ac_scale(p.H, p.up_h), y0, y1, wy);
      ac_coord(ix, p.W, ac_scale(p.W, p.up_w), x0, x1, wx);
      const h16* base = p.x + (long)bt[i] * p.H * p.W * p.Cin + ci;
      h8 a = __builtin_bit_cast(h8, ldg16(base + ((long)y0 * p.W + x0) * p.Cin));
      h8 b = __builtin_bit_cast(h8, ldg16(base + ((long)y0 * p.W + x1) * p.Cin));
      h8 c = __builtin_bit_cast(h8, ldg16(base + ((long)y1 * p.W + x0) * p.Cin));
      h8 d = __builtin_bit_cast(h8, ldg16(base + ((long)y1 * p.W + x1) * p.Cin));
      h8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float top = (float)a[j] + ((float)b[j] - (float)a[j]) * wx;
        float bot = (float)c[j] + ((float)d[j] - (float)c[j]) * wx;
        o[j] = (h16)(top + (bot - top) * wy);
      }
      v = __builtin_bit_cast(uint4, o);
    } else {
      if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) return make_uint4(0, 0, 0, 0);
      v = ldg16(p.x + (((long)bt[i] * p.H + iy) * p.W + ix) * p.Cin + ci);
    }
    if (p.pre_relu) v = relu_h8(v);
    return v;
  }
};

// ---- epilogue ------------------------------------------------------------------------------
// LayerNorm folded into the GEMM (vda_epilogue.ln_stats / ln_colsum): the row's (mean, rstd), from
// [M, 2] as is or from [M, ln_parts, 2] partial (sum, sumsq) over ln_parts column blocks
__device__ __forceinline__ float2 epi_ln_row(const GemmParams& p, int m) {
  const vda_epilogue& e = p.epi;
  if (e.ln_parts > 0) {
    float sm = 0.f, sq = 0.f;
    for (int t = 0; t < e.ln_parts; ++t) {
      const float2 pq = *reinterpret_cast<const float2*>(e.ln_stats + 2L * ((long)m * e.ln_parts + t));
      sm += pq.x;
      sq += pq.y;
    }
    const float mean = sm / (float)p.K;
    return make_float2(mean, rsqrtf(fmaxf(fmaf(-mean, mean, sq / (float)p.K), 0.f) + e.ln_eps));
  }
  return *reinterpret_cast<const float2*>(e.ln_stats + 2L * m);
}
template <int ACT>
__device__ __forceinline__ void epi_store4(const GemmParams& p, int m, int n, f4 v) {
  const vda_epilogue& e = p.epi;
  if (e.ln_stats) {  // LayerNorm folded into the GEMM: rstd * (acc - mean * colsum)
    const float2 mr = epi_ln_row(p, m);
    const f4 c1 = *reinterpret_cast<const f4*>(e.ln_colsum + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = mr.y * fmaf(-mr.x, c1[j], v[j]);
  }
  if (e.bias) {
    f4 b = *reinterpret_cast<const f4*>(e.bias + n);
    v += b;
  }
  if (e.rowbias) {
    int r = (m / e.rdiv) % e.rmod;
    f4 b = *reinterpret_cast<const f4*>(e.rowbias + (long)r * p.N + n);
    v += b;
  }
  if constexpr (ACT == VDA_ACT_GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
  } else if constexpr (ACT == VDA_ACT_RELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
  }
  if (e.gamma) {
    f4 g = *reinterpret_cast<const f4*>(e.gamma + n);
    v *= g;
  }
  if (e.res) {
    h4 r = *reinterpret_cast<const h4*>((const h16*)e.res + (long)m * e.ldres + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
  }
  if (e.res2) {
    h4 r = *reinterpret_cast<const h4*>((const h16*)e.res2 + (long)m * e.ldres2 + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
  }
  h4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (h16)v[j];
  long off;
  if (e.store == VDA_STORE_PIXEL_SHUFFLE) {
    int k = e.ps_k, cout = e.ps_cout;
    int ij = n / cout, co = n - ij * cout;
    int ki = ij / k, kj = ij - ki * k;
    int xw = m % e.ps_win;
    int t = m / e.ps_win;
    int yh = t % e.ps_hin;
    int bt = t / e.ps_hin;
    long oh = (long)yh * k + ki, ow = (long)xw * k + kj;
    off = (((long)bt * e.ps_hin * k + oh) * ((long)e.ps_win * k) + ow) * cout + co;
  } else {
    off = (long)m * p.ldy + n;
  }
  *reinterpret_cast<h4*>(p.y + off) = o;
}

// GEGLU / SwiGLU (ACT): h and g accumulators for the same 4 output channels.  Output column = n_out.
template <int ACT>
__device__ __forceinline__ void epi_geglu4(const GemmParams& p, int m, int nh, int ng, int n_out,
                                           f4 vh, f4 vg) {
  const vda_epilogue& e = p.epi;
  if (e.ln_stats) {  // LayerNorm folded in (the motion modules' ff_norm), on both halves before the gate
    const float2 mr = epi_ln_row(p, m);
    const f4 ch = *reinterpret_cast<const f4*>(e.ln_colsum + nh), cg = *reinterpret_cast<const f4*>(e.ln_colsum + ng);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vh[j] = mr.y * fmaf(-mr.x, ch[j], vh[j]);
      vg[j] = mr.y * fmaf(-mr.x, cg[j], vg[j]);
    }
  }
  if (e.bias) {
    vh += *reinterpret_cast<const f4*>(e.bias + nh);
    vg += *reinterpret_cast<const f4*>(e.bias + ng);
  }
  f4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = vh[j] * (ACT == VDA_ACT_SWIGLU ? silu_f32(vg[j]) : gelu_erf(vg[j]));
  const int nout_tot = p.N >> 1;
  if (e.gamma) v *= *reinterpret_cast<const f4*>(e.gamma + n_out);
  if (e.res) {
    h4 r = *reinterpret_cast<const h4*>((const h16*)e.res + (long)m * e.ldres + n_out);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
  }
  (void)nout_tot;
  h4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (h16)v[j];
  *reinterpret_cast<h4*>(p.y + (long)m * p.ldy + n_out) = o;
}

// ---- register-staged kernel (conv with a fused bilinear-upsample loader) ----------------------
template <int BM, int BN, class Loader, int ACT>
__global__ __launch_bounds__(256) void gemm_reg_kernel(GemmParams p, int tiles_n) {
  constexpr int TM = BM / 32;  // 16-row m subtiles per wave
  constexpr int TN = BN / 32;  // 16-row n subtiles per wave
  constexpr int XIT = BM / 32; // 16-B chunks per thread for the X tile (BM*8 / 256)
  constexpr int WIT = BN / 32;
  __shared__ __attribute__((aligned(16))) h16 sX[2][BM * BK];
  __shared__ __attribute__((aligned(16))) h16 sW[2][BN * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int tile_n = blockIdx.x % tiles_n, tile_m = blockIdx.x / tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  Loader ld;
  ld.init(p, m0, tid, XIT);
  const h16* wrow[WIT];
  bool wok[WIT];
#pragma unroll
  for (int i = 0; i < WIT; ++i) {
    int n = n0 + (tid >> 3) + 32 * i;
    wok[i] = n < p.N;
    wrow[i] = p.w + (long)(wok[i] ? n : 0) * p.K;
  }
  const int cchunk = tid & 7;

  uint4 rx[XIT], rw[WIT];
  auto gload = [&](int k0) {
    int k = k0 + cchunk * 8;
#pragma unroll
    for (int i = 0; i < XIT; ++i) rx[i] = ld.load(p, i, k);
#pragma unroll
    for (int i = 0; i < WIT; ++i) rw[i] = (wok[i] && k < p.K) ? ldg16(wrow[i] + k) : make_uint4(0, 0, 0, 0);
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XIT; ++i) *reinterpret_cast<uint4*>(&sX[buf][swz((tid >> 3) + 32 * i, cchunk)]) = rx[i];
#pragma unroll
    for (int i = 0; i < WIT; ++i) *reinterpret_cast<uint4*>(&sW[buf][swz((tid >> 3) + 32 * i, cchunk)]) = rw[i];
  };

  f4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + BK - 1) / BK;
  gload(0);
  sstore(0);
  __syncthreads();

  const int frow = lane & 15, fchunk = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * BK);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      h8 af[TN], bf[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i)
        af[i] = *reinterpret_cast<const h8*>(&sW[buf][swz(wn * (BN / 2) + i * 16 + frow, ks * 4 + fchunk)]);
#pragma unroll
      for (int j = 0; j < TM; ++j)
        bf[j] = *reinterpret_cast<const h8*>(&sX[buf][swz(wm * (BM / 2) + j * 16 + frow, ks * 4 + fchunk)]);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
    }
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds D[n = 4*(lane>>4) + r][m = lane&15] of every (i, j) subtile
  const int mcol = lane & 15, nq = (lane >> 4) * 4;
  if constexpr (vda_glu(ACT)) {
#pragma unroll
    for (int i = 0; i < TN; i += 2) {
      const int nbase = n0 + wn * (BN / 2) + i * 16;  // h block; gate block = nbase + 16
      if (nbase >= p.N) continue;
      const int n_out = (nbase >> 1) + nq;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        int m = m0 + wm * (BM / 2) + j * 16 + mcol;
        if (m < p.M) epi_geglu4<ACT>(p, m, nbase + nq, nbase + 16 + nq, n_out, acc[i][j], acc[i + 1][j]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + wn * (BN / 2) + i * 16 + nq;
      if (n >= p.N) continue;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        int m = m0 + wm * (BM / 2) + j * 16 + mcol;
        if (m < p.M) epi_store4<ACT>(p, m, n, acc[i][j]);
      }
    }
  }
}

// ---- LDS-DMA kernel (every dense GEMM and plain conv) ------------------------------------------
// Operand tiles are moved HBM -> LDS with global_load_lds_dwordx4 (no VGPR staging): one wave
// instruction fills 8 rows x 128 B of the [BM + BN][64] tile (X rows first, then W rows).  The DMA
// destination is lane-linear, so the (row>>1)&7 chunk swizzle is applied to the per-lane SOURCE
// address.  Lanes whose source is out of range (rows >= M / N, k >= K, conv zero padding) read a
// zero page instead, so no predication reaches the LDS image.  Two LDS buffers, BK = 64: tile t+1
// is issued before the MFMAs of tile t and drained by the barrier that ends tile t.
// Block -> tile mapping is XCD-aware: the 8 XCDs each take a contiguous run of tiles, grouped
// GROUP_M m-panels at a time so co-resident blocks share X panels and W tiles in their XCD's L2.
__device__ __attribute__((aligned(64))) uint4 g_zero_page[4];

#ifndef VDA_GROUP_M  // (A/B builds only)
#define VDA_GROUP_M 8
#endif
constexpr int GROUP_M = VDA_GROUP_M;  // m-panels per XCD tile group (2 / 4 / 16 within noise: profiles/r04_ab_gemm_group_m.log)
constexpr int ACT_DEPTH = 100;  // internal (outside the VDA_ACT_* codes): depth-head tail epilogue (vda_depth_head)

__device__ __forceinline__ void tile_coords(int bid, int nwg, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int per_group = GROUP_M * tiles_n;
  const int group = wgid / per_group;
  const int first_m = group * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int in_group = wgid - group * per_group;
  tm = first_m + in_group % gsize;
  tn = in_group / gsize;
}

template <int KB>
__device__ __forceinline__ int swzk(int row, int chunk) {  // half offset in a [rows][KB] tile
  constexpr int CH = KB / 8;
  return row * KB + ((chunk ^ ((row >> 1) & (CH - 1))) << 3);
}

// NS-stage LDS-DMA pipeline: tile kt+NS-1 is issued while tile kt is multiplied; before reading a
// stage every wave waits with a COUNTED vmcnt (its own newer pieces stay in flight) and passes a
// raw s_barrier (no __syncthreads: its fence would drain every DMA in flight).
template <int BM, int BN, int NWM, int NWN, int KB, int NS, bool CONV, int ACT>
__global__ __launch_bounds__(NWM * NWN * 64) void gemm_kernel(GemmParams p, int tiles_m, int tiles_n) {
  constexpr int NW = NWM * NWN;
  constexpr int WTM = BM / NWM, WTN = BN / NWN;  // wave tile
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int ROWS = BM + BN;
  constexpr int CH = KB / 8;                     // 16-B chunks per row
  constexpr int RPP = 64 / CH;                   // rows per 1-KiB DMA piece
  constexpr int GROUPS = ROWS / RPP;             // pieces per stage
  static_assert(GROUPS % NW == 0, "pieces must divide evenly over the waves");
  constexpr int IPW = GROUPS / NW;               // DMA instructions per wave per stage
  constexpr int STAGE = ROWS * KB;               // halfs per stage
  __shared__ __attribute__((aligned(1024))) h16 smem[NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % NWM, wn = wave / NWM;
  int tile_m, tile_n;
  tile_coords(blockIdx.x, gridDim.x, tiles_m, tiles_n, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // per-lane source descriptors for this wave's IPW pieces
  const h16* rowp[IPW];
  int kch[IPW];        // logical k offset (halfs) of this lane's chunk within the K tile
  bool isx[IPW];
  int cbt[IPW], coy[IPW], cox[IPW];
  bool rowok[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int g = wave * IPW + i;
    const int R = g * RPP + lane / CH;
    const int c = (lane % CH) ^ ((R >> 1) & (CH - 1));
    kch[i] = c * 8;
    isx[i] = R < BM;
    if (R < BM) {
      const int m = m0 + R;
      rowok[i] = m < p.M;
      if constexpr (CONV) {
        const int mm = rowok[i] ? m : 0;
        cox[i] = mm % p.Wo;
        const int t = mm / p.Wo;
        coy[i] = t % p.Ho;
        cbt[i] = t / p.Ho;
        rowp[i] = p.x;
      } else {
        rowp[i] = p.x + (long)(rowok[i] ? m : 0) * p.ldx;
      }
    } else {
      const int n = n0 + R - BM;
      rowok[i] = n < p.N;
      rowp[i] = p.w + (long)(rowok[i] ? n : 0) * p.K;
    }
  }
  const void* zero = (const void*)g_zero_page;

  auto issue = [&](int k0, int buf) {
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int k = k0 + kch[i];
      const void* src = zero;
      if (rowok[i] && k < p.K) {
        if (CONV && isx[i]) {
          const int tap = k / p.Cin, ci = k - tap * p.Cin;
          const int ky = tap / p.ks, kx = tap - ky * p.ks;
          const int iy = coy[i] * p.stride - p.pad + ky, ix = cox[i] * p.stride - p.pad + kx;
          if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
            src = p.x + (((long)cbt[i] * p.H + iy) * p.W + ix) * p.Cin + ci;
        } else {
          src = rowp[i] + k;
        }
      }
      glds16(src, smem + buf * STAGE + (wave * IPW + i) * RPP * KB);
    }
  };

  f4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + KB - 1) / KB;
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) issue(s * KB, s);
  const int frow = lane & 15, fchunk = lane >> 4;
  const bool prerelu = CONV && p.pre_relu;
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt must have landed; the (up to NS-2) newer tiles may stay in flight
    const int newer = min(NS - 2, nk - 1 - kt);
    if constexpr (NS >= 4) {
      if (newer >= 2) wait_vmcnt<2 * IPW>();
      else if (newer == 1) wait_vmcnt<IPW>();
      else wait_vmcnt<0>();
    } else if constexpr (NS == 3) {
      if (newer >= 1) wait_vmcnt<IPW>();
      else wait_vmcnt<0>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    {
      const int nxt = kt + NS - 1;
      if (nxt < nk) issue(nxt * KB, nxt % NS);
    }
    const h16* sX = smem + buf * STAGE;
    const h16* sW = sX + BM * KB;
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks) {
      h8 af[TN], bf[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i)
        af[i] = *reinterpret_cast<const h8*>(&sW[swzk<KB>(wn * WTN + i * 16 + frow, ks * 4 + fchunk)]);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        bf[j] = *reinterpret_cast<const h8*>(&sX[swzk<KB>(wm * WTM + j * 16 + frow, ks * 4 + fchunk)]);
        if (prerelu) bf[j] = relu8(bf[j]);
      }
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
    }
    buf = (buf + 1 == NS) ? 0 : buf + 1;
  }

  const int mcol = lane & 15, nq = (lane >> 4) * 4;
  if constexpr (ACT == ACT_DEPTH) {
    // depth tail (dpt.py:118-124): the wave owns all 64 W rows = 32 output channels as fp16
    // hi (rows 0..31) + lo (rows 32..63) halves of the fp32 weights, so y = acc_hi + acc_lo is the
    // fp32-weight conv.  Then +b1, ReLU, 1x1 (32 -> 1) dot, +b2, ReLU; fp32 depth per pixel.
    static_assert(TN == 4 && NWN == 1, "depth epilogue needs the whole 64-row W tile per wave");
    const float* b1 = p.epi.bias;
    const float* w2 = p.epi.gamma;
    const float b2 = p.epi.rowbias[0];
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = i * 16 + nq + r;
          const float y = acc[i][j][r] + acc[i + 2][j][r] + b1[c];
          part += fmaxf(y, 0.f) * w2[c];
        }
      part += __shfl_xor(part, 16, 64);
      part += __shfl_xor(part, 32, 64);
      const int m = m0 + wm * WTM + j * 16 + mcol;
      if (lane < 16 && m < p.M) reinterpret_cast<float*>(p.y)[m] = fmaxf(part + b2, 0.f);
    }
  } else if constexpr (vda_glu(ACT)) {
    static_assert(TN % 2 == 0, "GEGLU / SwiGLU needs an even number of n subtiles per wave");
#pragma unroll
    for (int i = 0; i < TN; i += 2) {
      const int nbase = n0 + wn * WTN + i * 16;
      if (nbase >= p.N) continue;
      const int n_out = (nbase >> 1) + nq;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int m = m0 + wm * WTM + j * 16 + mcol;
        if (m < p.M) epi_geglu4<ACT>(p, m, nbase + nq, nbase + 16 + nq, n_out, acc[i][j], acc[i + 1][j]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + wn * WTN + i * 16 + nq;
      if (n >= p.N) continue;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int m = m0 + wm * WTM + j * 16 + mcol;
        if (m < p.M) epi_store4<ACT>(p, m, n, acc[i][j]);
      }
    }
  }
}

}  // namespace
