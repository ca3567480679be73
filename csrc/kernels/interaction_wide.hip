// DLRM dot feature interaction for 33..64 features ("wide" form of interaction.hip): the per-sample
// feature matrix Z is two 32-row MFMA halves, Z0 = rows 0..31 and Z1 = rows 32..63 (rows >= F unused).
//
// Forward, one wave per sample: G00 = Z0 Z0^T, G10 = Z1 Z0^T, G11 = Z1 Z1^T (the upper-right tile
//   holds no pair j < i) on v_mfma_f32_32x32x16_bf16, 48 accumulator registers.  Lane (r, h) holds
//   Z[r][16ks + 8h .. +7] and Z[32 + r][same] straight from global memory.  fp32 inputs go through
//   the exact three-way bf16 split of common.h (six plane products per tile, small terms first), so
//   the result is fp32-accurate at a quarter of the fp32 MFMA's cycles.  The k-steps live in S
//   register slots: a slot is reloaded with the NEXT work item's fragment right after its MFMAs, so
//   one sample's loads are always in flight behind the compute; D > 128 runs as two chunks of 8
//   slots.  The row [x | triangle | pad] is assembled in a per-wave LDS row, written with 16-B stores.
// Backward dZ = S Z, S = dG + dG^T gathered from the staged dOut row through per-lane positions
//   packed two to a register and computed once; zero entries point at a zero slot behind the row and
//   the self-interaction diagonal is doubled in place in LDS, so the gather is a plain LDS read.
//   bf16: Z (64 x <=128 columns) staged in LDS, B operand by ds_read_b64_tr_b16, the two 32-row
//   output halves one after the other (<= 64 accumulators), each through an LDS transpose to 16-B
//   stores; D > 128 as two column chunks (columns of dZ are independent).
//   fp32: v_mfma_f32_32x32x2_f32 with the B operand straight from global memory in 64-column
//   chunks: whole row segments with wave-uniform pointers, put into operand (and, for the stores,
//   whole-row) order by v_permlane32_swap; the register set is reloaded in place with the next chunk.
// Supported: 33 <= F <= 64, D % 16 == 0, D <= 256, 16-B aligned bases and row strides.
#include "common.h"

#include <algorithm>

namespace {

constexpr int MAXFW = 64;
template <typename T> struct WTab {
  const T* p[MAXFW];
};
template <typename T> struct WMTab {
  T* p[MAXFW];
};
typedef unsigned short bf16_t;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) bf16x4_t lds_v4_t;

FM_DEVICE int pair_pos(int i, int j, int self) { return self ? (i * (i + 1) / 2 + j) : (i * (i - 1) / 2 + j); }

// index in the staged dOut row of S[i][j]; `zero` (the zero slot) for an entry that is 0
FM_DEVICE unsigned s_pos(int i, int j, int F, int D, int self, int zero) {
  if (i >= F || j >= F || (i == j && !self)) return (unsigned)zero;
  return (unsigned)(D + (i >= j ? pair_pos(i, j, self) : pair_pos(j, i, self)));
}

// ---- forward ------------------------------------------------------------------------------------
// 8 consecutive k of one Z row: the operand fragment of one 16-k MFMA step
template <typename T> struct Frag8;
template <> struct Frag8<bf16_t> {
  bf16x8_t v;
};
template <> struct Frag8<float> {
  f32x4_t a, b;
};
FM_DEVICE Frag8<bf16_t> ldfrag(const bf16_t* p) { return {*reinterpret_cast<const bf16x8_t*>(p)}; }
FM_DEVICE Frag8<float> ldfrag(const float* p) {
  return {*reinterpret_cast<const f32x4_t*>(p), *reinterpret_cast<const f32x4_t*>(p + 4)};
}
FM_DEVICE void stfrag(bf16_t* p, const Frag8<bf16_t>& f) { *reinterpret_cast<bf16x8_t*>(p) = f.v; }
FM_DEVICE void stfrag(float* p, const Frag8<float>& f) {
  *reinterpret_cast<f32x4_t*>(p) = f.a;
  *reinterpret_cast<f32x4_t*>(p + 4) = f.b;
}

#define FM_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

FM_DEVICE void gram_step(const Frag8<bf16_t>& a0, const Frag8<bf16_t>& a1, f32x16_t& g00, f32x16_t& g10, f32x16_t& g11) {
  const bf16x8v_t x0 = __builtin_bit_cast(bf16x8v_t, a0.v), x1 = __builtin_bit_cast(bf16x8v_t, a1.v);
  g00 = FM_MFMA_BF16(x0, x0, g00);
  g10 = FM_MFMA_BF16(x1, x0, g10);
  g11 = FM_MFMA_BF16(x1, x1, g11);
}

struct Planes {
  bf16x8v_t h, m, l;
};
FM_DEVICE Planes split3(const Frag8<float>& f) {
  unsigned ph[4], pm[4], pl[4];
  fm_split3_pair(f.a[0], f.a[1], ph[0], pm[0], pl[0]);
  fm_split3_pair(f.a[2], f.a[3], ph[1], pm[1], pl[1]);
  fm_split3_pair(f.b[0], f.b[1], ph[2], pm[2], pl[2]);
  fm_split3_pair(f.b[2], f.b[3], ph[3], pm[3], pl[3]);
  return {__builtin_bit_cast(bf16x8v_t, u32x4_t{ph[0], ph[1], ph[2], ph[3]}),
          __builtin_bit_cast(bf16x8v_t, u32x4_t{pm[0], pm[1], pm[2], pm[3]}),
          __builtin_bit_cast(bf16x8v_t, u32x4_t{pl[0], pl[1], pl[2], pl[3]})};
}
// the six plane products with indices summing to <= 2, small terms first, the three tiles interleaved
// so that no MFMA waits for the one before it
FM_DEVICE void gram_step(const Frag8<float>& a0, const Frag8<float>& a1, f32x16_t& g00, f32x16_t& g10, f32x16_t& g11) {
  const Planes p0 = split3(a0), p1 = split3(a1);
#define FM_WIDE_TERM(A, Bp)              \
  g00 = FM_MFMA_BF16(p0.A, p0.Bp, g00);  \
  g10 = FM_MFMA_BF16(p1.A, p0.Bp, g10);  \
  g11 = FM_MFMA_BF16(p1.A, p1.Bp, g11);
  FM_WIDE_TERM(l, h)
  FM_WIDE_TERM(h, l)
  FM_WIDE_TERM(m, m)
  FM_WIDE_TERM(m, h)
  FM_WIDE_TERM(h, m)
  FM_WIDE_TERM(h, h)
#undef FM_WIDE_TERM
}

// S register slots of one k-step each, C chunks of S k-steps per sample (D <= 16 S C)
template <typename T, int S, int C>
__global__ void __launch_bounds__(256) fm_dotw_fwd(WTab<T> Z, long ldz, T* __restrict__ out, long ldo, long B, int F,
                                                   int D, int W, int self) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int VE = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T* row = reinterpret_cast<T*>(smem) + (long)wave * W;          // W % VE == 0: rows stay 16-B aligned
  const int waves_total = gridDim.x * (blockDim.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int ksn = D >> 4;
  const int npairs = self ? F * (F + 1) / 2 : F * (F - 1) / 2;
  // rows >= F read row 0: their Gram rows and columns are never written out
  const T* z0 = Z.p[r] + 8 * h;
  const T* z1 = Z.p[32 + r < F ? 32 + r : 0] + 8 * h;
  Frag8<T> f0[S], f1[S];
  auto load = [&](long bb, int c, int s) {     // k-steps past D reload the last one (unconditional loads)
    const int ks = min(c * S + s, ksn - 1);
    f0[s] = ldfrag(z0 + bb * ldz + 16 * ks);
    f1[s] = ldfrag(z1 + bb * ldz + 16 * ks);
  };
  long b = blockIdx.x * (blockDim.x >> 6) + wave;
  {
    const long b0 = min(b, B - 1);
#pragma unroll
    for (int s = 0; s < S; ++s) load(b0, 0, s);
  }
  for (; b < B; b += waves_total) {
    const long bn = min(b + waves_total, B - 1);
    f32x16_t g00, g10, g11;
#pragma unroll
    for (int i = 0; i < 16; ++i) g00[i] = g10[i] = g11[i] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int ks = c * S + s;
        if (ks < ksn) {                                           // uniform
          gram_step(f0[s], f1[s], g00, g10, g11);
          if (r == 0) stfrag(row + 16 * ks + 8 * h, f0[s]);       // lanes 0 / 32 hold row 0 = x
        }
        if (c + 1 < C) load(b, c + 1, s);
        else load(bn, 0, s);
        __builtin_amdgcn_sched_barrier(0);   // keep the reload between this step's MFMAs and the next's
      }
    }
    for (int c = D + npairs + lane; c < W; c += 64) row[c] = fromf<T>(0.f);
    // lane holds G[i][j] of each tile at i = (q&3) + 8(q>>2) + 4h, j = lane&31
    T* tri = row + D;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
      if (self ? r <= i : r < i) tri[pair_pos(i, r, self)] = fromf<T>(g00[q]);
      if (32 + i < F) {
        tri[pair_pos(32 + i, r, self)] = fromf<T>(g10[q]);
        if (self ? r <= i : r < i) tri[pair_pos(32 + i, 32 + r, self)] = fromf<T>(g11[q]);
      }
    }
    FM_WAVE_LDS_SYNC();
    T* o = out + b * ldo;
    for (int c = lane * VE; c < W; c += 64 * VE) *reinterpret_cast<u32x4_t*>(o + c) = *reinterpret_cast<const u32x4_t*>(row + c);
    FM_WAVE_LDS_SYNC();
  }
}

// ---- bf16 backward ------------------------------------------------------------------------------
// DC columns of Z per chunk (LDS image [64][DC]), NC chunks per sample (D <= DC NC)
template <int DC, int NC>
__global__ void __launch_bounds__(256) fm_dotw_bwd(WTab<bf16_t> Z, long ldz, const bf16_t* __restrict__ dout, long ldo,
                                                   WMTab<bf16_t> dZ, long lddz, unsigned long long acc_mask, long B,
                                                   int F, int D, int W, int self) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CPRM = DC / 8;          // lanes (16-B chunks) per staged row
  constexpr int RPI = 64 / CPRM;        // rows per wave-wide access
  constexpr int NI = 64 / RPI;          // accesses for the 64 rows of Z
  constexpr int NT = DC / 32;
  constexpr int DCH = 5;                // 16-B chunks of the dOut row per lane (W <= 2560)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bf16_t* zs = reinterpret_cast<bf16_t*>(smem) + (long)wave * (96 * DC + W + 8);   // Z chunk [64][DC]
  bf16_t* os = zs + 64 * DC;                                                       // dZ half tile [32][DC]
  bf16_t* ds = os + 32 * DC;                                                       // dOut row [W] + zero slot
  const int waves_total = gridDim.x * (blockDim.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int lc = lane % CPRM, lr = lane / CPRM;
  // A operand of row half rh, k-step ks: S[32rh + r][16ks + 8h + e], e = 0..7, as dOut-row positions
  unsigned apk[2][4][4];
#pragma unroll
  for (int rh = 0; rh < 2; ++rh)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = 16 * ks + 8 * h + 2 * u;
        apk[rh][ks][u] = s_pos(32 * rh + r, j, F, D, self, W) | (s_pos(32 * rh + r, j + 1, F, D, self, W) << 16);
      }
  if (lane < 8) ds[W + lane] = 0;
  // persistent waves: the next work item's Z chunk and the next sample's dOut row are in flight in
  // registers (clamped addresses, every load unconditional) while this one is staged and multiplied
  u32x4_t zv[NI], dv[DCH];
  auto load_z = [&](long bb, int c) {
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int j = t * RPI + lr, k = c * DC + 8 * lc;
      const bool ok = j < F && k < D;
      zv[t] = *reinterpret_cast<const u32x4_t*>(Z.p[ok ? j : 0] + bb * ldz + (ok ? k : 0));
    }
  };
  auto load_d = [&](long bb) {
#pragma unroll
    for (int t = 0; t < DCH; ++t) {
      const int c8 = 8 * (lane + 64 * t);
      dv[t] = *reinterpret_cast<const u32x4_t*>(dout + bb * ldo + (c8 < W ? c8 : 0));
    }
  };
  long b = blockIdx.x * (blockDim.x >> 6) + wave;
  {
    const long b0 = min(b, B - 1);
    load_z(b0, 0);
    load_d(b0);
  }
  const int g = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  for (; b < B; b += waves_total) {
    const long bn = min(b + waves_total, B - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col0 = c * DC;
#pragma unroll
      for (int t = 0; t < NI; ++t) {       // rows >= F and columns >= D are zero in the LDS image
        const int j = t * RPI + lr;
        const bool ok = j < F && col0 + 8 * lc < D;
        *reinterpret_cast<u32x4_t*>(zs + j * DC + 8 * lc) = ok ? zv[t] : u32x4_t{0u, 0u, 0u, 0u};
      }
      if (c == 0) {
#pragma unroll
        for (int t = 0; t < DCH; ++t) {
          const int c8 = 8 * (lane + 64 * t);
          if (c8 < W) *reinterpret_cast<u32x4_t*>(ds + c8) = dv[t];
        }
      }
      FM_WAVE_LDS_SYNC();
      if (c == 0) load_d(bn);
      if (c + 1 < NC) load_z(b, c + 1);
      else load_z(bn, 0);
      if (c == 0 && self) {                // S_ii = 2 dG_ii: doubled in place (no other reader)
        if (lane < F) {
          bf16_t* d = ds + D + pair_pos(lane, lane, 1);
          *d = f2bf(2.f * bf2f(*d));
        }
        FM_WAVE_LDS_SYNC();
      }
#pragma unroll
      for (int rh = 0; rh < 2; ++rh) {
        bf16x8_t afr[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const unsigned pk = apk[rh][ks][u];
            afr[ks][2 * u] = (short)ds[pk & 0xffffu];
            afr[ks][2 * u + 1] = (short)ds[pk >> 16];
          }
        f32x16_t acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (col0 + 32 * nt >= D) continue;                      // uniform
#pragma unroll
          for (int t = 0; t < 16; ++t) acc[nt][t] = 0.f;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const int krow = 16 * ks + 8 * (g >> 1) + q4;
            const int col = 32 * nt + 16 * (g & 1) + 4 * p4;
            bf16x8_t bb;
            bb.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(zs + krow * DC + col));
            bb.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(zs + (krow + 4) * DC + col));
            acc[nt] = FM_MFMA_BF16(__builtin_bit_cast(bf16x8v_t, afr[ks]), __builtin_bit_cast(bf16x8v_t, bb), acc[nt]);
          }
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const int i = (t & 3) + 8 * (t >> 2) + 4 * h;
            os[i * DC + 32 * nt + r] = f2bf(acc[nt][t]);
          }
        }
        FM_WAVE_LDS_SYNC();
#pragma unroll
        for (int t = 0; t < NI / 2; ++t) {
          const int i = t * RPI + lr, gi = 32 * rh + i, col = col0 + 8 * lc;
          bf16_t* d = dZ.p[gi];                                   // nullptr for gi >= F
          if (d == nullptr || col >= D) continue;
          d += b * lddz + col;
          bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(os + i * DC + 8 * lc);
          const bool add_x = gi == 0, add_old = (acc_mask >> gi) & 1ull;
          if (add_x || add_old) {
            const bf16x8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};
            const bf16x8_t x = add_x ? *reinterpret_cast<const bf16x8_t*>(ds + col) : z8;
            const bf16x8_t o = add_old ? *reinterpret_cast<const bf16x8_t*>(d) : z8;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              v[e] = (short)f2bf(bf2f((bf16_t)v[e]) + bf2f((bf16_t)x[e]) + bf2f((bf16_t)o[e]));
          }
          *reinterpret_cast<bf16x8_t*>(d) = v;
        }
        FM_WAVE_LDS_SYNC();
      }
    }
  }
}

// ---- fp32 backward ------------------------------------------------------------------------------
// a = [a.lo | b.lo], b = [a.hi | b.hi] over the two 32-lane halves of the wave (v_permlane32_swap)
FM_DEVICE void half_swap(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

// Every global access is one whole 64-column row segment with a wave-uniform row pointer: lane l
// loads Z[j][64c + l]; a half swap of rows 2ks and 2ks + 1 gives the B operands of the two column
// tiles (lane (r, h): Z[2ks + h][64c + 32e + r]), and a half swap of the two tiles' accumulators
// gives whole rows i0 and i0 + 4 of dZ for the stores.
__global__ void __launch_bounds__(256) fm_dotw_bwd_f32(WTab<float> Z, long ldz, const float* __restrict__ dout, long ldo,
                                                       WMTab<float> dZ, long lddz, unsigned long long acc_mask, long B,
                                                       int F, int D, int W, int self, int act0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = 32;               // k-steps of 2 rows of Z
  constexpr int DCH = 10;               // float4 chunks of the dOut row per lane (W <= 2560)
  // the wave index as a scalar: sample offsets then fold into the wave-uniform row pointers and
  // every global access is an SGPR base plus one 32-bit lane offset
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* ds = reinterpret_cast<float*>(smem) + (long)wave * (W + 4);   // dOut row [W] + zero slot
  const int waves_total = gridDim.x * (blockDim.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nks = (F + 1) / 2, NC = (D + 63) / 64;
  // A operands of k-step ks: S[r][2ks + h] (low half) and S[32 + r][2ks + h] (high half)
  unsigned apk[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    apk[ks] = s_pos(r, 2 * ks + h, F, D, self, W) | (s_pos(32 + r, 2 * ks + h, F, D, self, W) << 16);
  if (lane < 4) ds[W + lane] = 0.f;
  // zn[j] holds Z[j][64c + lane] of the CURRENT chunk and is reloaded with the next chunk's (or the
  // next sample's first) right after its MFMAs are issued; rows >= F reload row F - 1 and columns
  // >= D column 0, so every load is unconditional and the vmcnt waits stay exact
  float zn[2 * NKS];
  f32x4_t dn[DCH];
  auto load_row = [&](long bb, int c, int j) {
    const unsigned col = 64 * c + lane;
    zn[j] = (Z.p[min(j, F - 1)] + bb * ldz)[col < D ? col : 0u];
  };
  auto load_dout = [&](long bb) {
#pragma unroll
    for (int t = 0; t < DCH; ++t) {
      const unsigned c4 = 4 * (lane + 64 * t);
      dn[t] = *reinterpret_cast<const f32x4_t*>((dout + bb * ldo) + (c4 < W ? c4 : 0u));
    }
  };
  long b = blockIdx.x * (blockDim.x >> 6) + wave;
  {
    const long b0 = min(b, B - 1);
#pragma unroll
    for (int j = 0; j < 2 * NKS; ++j) load_row(b0, 0, j);
    load_dout(b0);
  }
  for (; b < B; b += waves_total) {
    const long bn = min(b + waves_total, B - 1);
#pragma unroll
    for (int t = 0; t < DCH; ++t) {
      const int c4 = 4 * (lane + 64 * t);
      if (c4 < W) *reinterpret_cast<f32x4_t*>(ds + c4) = dn[t];
    }
    FM_WAVE_LDS_SYNC();
    load_dout(bn);
    if (self) {                          // S_ii = 2 dG_ii: doubled in place (no other reader)
      if (lane < F) ds[D + pair_pos(lane, lane, 1)] *= 2.f;
      FM_WAVE_LDS_SYNC();
    }
    for (int c = 0; c < NC; ++c) {
      const bool last = c + 1 == NC;
      const long lb = last ? bn : b;
      const int lcn = last ? 0 : c + 1;
      const unsigned col = 64 * c + lane;
      const bool cok = col < D;
      const float x0 = ds[cok ? col : 0];   // dZ_0 += dOut[:, :D]
      const float z0 = zn[0];               // row 0 of this chunk (for act0; zn is reloaded below)
      f32x16_t acc[2][2];
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[0][0][t] = acc[0][1][t] = acc[1][0][t] = acc[1][1][t] = 0.f;
      float a0 = ds[apk[0] & 0xffffu], a1 = ds[apk[0] >> 16];
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        float n0 = 0.f, n1 = 0.f;        // the next step's S entries, gathered behind this step's MFMAs
        if (ks + 1 < NKS) {
          n0 = ds[apk[ks + 1] & 0xffffu];
          n1 = ds[apk[ks + 1] >> 16];
        }
        if (ks < nks) {                  // uniform: steps past F are skipped, not padded
          float u = zn[2 * ks], v = zn[2 * ks + 1];
          half_swap(u, v);               // u: rows 2ks + h at columns 64c + r, v: at 64c + 32 + r
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, u, acc[0][0], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, u, acc[1][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, v, acc[0][1], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, v, acc[1][1], 0, 0, 0);
        }
        load_row(lb, lcn, 2 * ks);
        load_row(lb, lcn, 2 * ks + 1);
        a0 = n0;
        a1 = n1;
        __builtin_amdgcn_sched_barrier(0);
      }
      // row i of dZ at columns 64c + lane (i, the pointer and the accumulate flag are wave-uniform)
      auto store_row = [&](int i, float v) {
        if (i >= F || dZ.p[i] == nullptr) return;
        if (i == 0) {
          v += x0;
          // activation backward of feature 0's producer (see interaction.hip)
          if (act0 != ACT_NONE) v = act_bwd(act0, z0, v);
        }
        if (cok) {
          float* d = (dZ.p[i] + b * lddz) + col;
          if ((acc_mask >> i) & 1ull) v += *d;
          *d = v;
        }
      };
#pragma unroll
      for (int rh = 0; rh < 2; ++rh)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int i0 = 32 * rh + (t & 3) + 8 * (t >> 2);     // lanes h hold row i0 + 4h of both tiles
          float c0 = acc[rh][0][t], c1 = acc[rh][1][t];
          half_swap(c0, c1);
          store_row(i0, c0);
          store_row(i0 + 4, c1);
        }
    }
    FM_WAVE_LDS_SYNC();
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// which condition of the wide form fails (fm_dot_interaction_error names it), 0 = none
template <typename T>
int wide_status(const void* const* z, void* const* dz, int F, long ldz, const void* o, long ldo, long lddz, int D, int W) {
  constexpr int VE = 16 / (int)sizeof(T);
  if (F < 33 || F > MAXFW) return FM_DOT_FEATURES;
  if (D < 16 || D % 16 != 0 || D > 256) return FM_DOT_WIDE_D;
  if (W % VE != 0 || W > 2560) return FM_DOT_WIDE_W;
  bool ok = ldz % VE == 0 && ldo % VE == 0 && lddz % VE == 0 && al16(o);
  for (int i = 0; i < F; ++i) ok = ok && al16(z[i]) && (dz == nullptr || al16(dz[i]));
  return ok ? 0 : FM_DOT_WIDE_ALIGN;
}

template <typename K> void big_lds(K k) {
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 << 10);
}

template <typename T>
int wide_fwd(const void* const* z, int F, long ldz, void* out, long ldo, long B, int D, int W, int self, hipStream_t s) {
  const int npairs = self ? F * (F + 1) / 2 : F * (F - 1) / 2;
  if (int st = wide_status<T>(z, nullptr, F, ldz, out, ldo, 0, D, W)) return st;
  if (W < D + npairs) return FM_DOT_WIDE_W;
  if (B <= 0) return 0;
  WTab<T> t;
  for (int i = 0; i < MAXFW; ++i) t.p[i] = i < F ? (const T*)z[i] : nullptr;
  const int waves = 4;
  const long blocks = std::min<long>((B + waves - 1) / waves, fm_dot_block_cap());
  auto k = D <= 32 ? fm_dotw_fwd<T, 2, 1> : D <= 64 ? fm_dotw_fwd<T, 4, 1> : D <= 128 ? fm_dotw_fwd<T, 8, 1>
                                                                                     : fm_dotw_fwd<T, 8, 2>;
  hipLaunchKernelGGL(k, dim3((int)blocks), dim3(64 * waves), (size_t)waves * W * sizeof(T), s, t, ldz, (T*)out, ldo, B,
                     F, D, W, self);
  return 0;
}

}  // namespace

extern "C" void fm_dot_interaction_error(int status, const char** msg) {
  *msg = status == 0                   ? "ok"
         : status == FM_DOT_FEATURES   ? "dot interaction: 1..64 features"
         : status == FM_DOT_WIDE_D     ? "dot interaction with more than 32 features: D % 16 == 0 and D <= 256"
         : status == FM_DOT_WIDE_W     ? "dot interaction with more than 32 features: row width a multiple of 16 bytes, "
                                         "at least D + pairs and at most 2560 elements"
         : status == FM_DOT_WIDE_ALIGN ? "dot interaction with more than 32 features: 16-byte aligned bases and row "
                                         "strides (ld % 8 for bf16, ld % 4 for fp32)"
                                       : "dot interaction: unknown status";
}

extern "C" int fm_dot_interaction_wide_fwd(const void* const* z, int F, long ldz, void* out, long ldo, long B, int D, int W,
                                           int self, hipStream_t s) {
  return wide_fwd<bf16_t>(z, F, ldz, out, ldo, B, D, W, self, s);
}

extern "C" int fm_dot_interaction_wide_fwd_f32(const float* const* z, int F, long ldz, float* out, long ldo, long B, int D,
                                               int W, int self, hipStream_t s) {
  return wide_fwd<float>((const void* const*)z, F, ldz, out, ldo, B, D, W, self, s);
}

extern "C" int fm_dot_interaction_wide_bwd(const void* const* z, int F, long ldz, const void* dout, long ldo,
                                           void* const* dz, long lddz, unsigned long long acc_mask, long B, int D,
                                           int self, hipStream_t s) {
  const int npairs = self ? F * (F + 1) / 2 : F * (F - 1) / 2;
  const int W = (D + npairs + 7) & ~7;      // dOut columns read (x part + packed triangle)
  if (int st = wide_status<bf16_t>(z, dz, F, ldz, dout, ldo, lddz, D, W)) return st;
  if (B <= 0) return 0;
  WTab<bf16_t> t;
  WMTab<bf16_t> g;
  for (int i = 0; i < MAXFW; ++i) {
    t.p[i] = i < F ? (const bf16_t*)z[i] : nullptr;
    g.p[i] = i < F ? (bf16_t*)dz[i] : nullptr;
  }
  const int waves = 4;
  const long blocks = std::min<long>((B + waves - 1) / waves, fm_dot_block_cap());
  static bool attr = false;
  if (!attr) {
    big_lds(fm_dotw_bwd<32, 1>);
    big_lds(fm_dotw_bwd<64, 1>);
    big_lds(fm_dotw_bwd<128, 1>);
    big_lds(fm_dotw_bwd<128, 2>);
    attr = true;
  }
  const int DC = D <= 32 ? 32 : D <= 64 ? 64 : 128;
  auto k = D <= 32 ? fm_dotw_bwd<32, 1> : D <= 64 ? fm_dotw_bwd<64, 1> : D <= 128 ? fm_dotw_bwd<128, 1> : fm_dotw_bwd<128, 2>;
  const size_t lds = (size_t)waves * (96 * DC + W + 8) * 2;
  hipLaunchKernelGGL(k, dim3((int)blocks), dim3(64 * waves), lds, s, t, ldz, (const bf16_t*)dout, ldo, g, lddz, acc_mask,
                     B, F, D, W, self);
  return 0;
}

extern "C" int fm_dot_interaction_wide_bwd_f32(const float* const* z, int F, long ldz, const float* dout, long ldo,
                                               float* const* dz, long lddz, unsigned long long acc_mask, long B, int D,
                                               int self, int act0, hipStream_t s) {
  const int npairs = self ? F * (F + 1) / 2 : F * (F - 1) / 2;
  const int W = (D + npairs + 3) & ~3;      // dOut columns read
  if (int st = wide_status<float>((const void* const*)z, (void* const*)dz, F, ldz, dout, ldo, lddz, D, W)) return st;
  if (B <= 0) return 0;
  WTab<float> t;
  WMTab<float> g;
  for (int i = 0; i < MAXFW; ++i) {
    t.p[i] = i < F ? z[i] : nullptr;
    g.p[i] = i < F ? dz[i] : nullptr;
  }
  const int waves = 4;
  const long blocks = std::min<long>((B + waves - 1) / waves, fm_dot_block_cap());
  hipLaunchKernelGGL(fm_dotw_bwd_f32, dim3((int)blocks), dim3(64 * waves), (size_t)waves * (W + 4) * 4, s, t, ldz, dout,
                     ldo, g, lddz, acc_mask, B, F, D, W, self, act0);
  return 0;
}
