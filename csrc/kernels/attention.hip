// Fused multi-head attention, O = softmax(scale Q K^T + mask) V per (batch, head), flash style: no
// [Tq, Tk] matrix ever reaches global memory, the only state kept for the backward is the per-row
// log-sum-exp.  q/k/v/o are [B, T, heads * DH] with head h at columns [h DH, (h + 1) DH) (the layout a
// Linear writes), every operand is a base pointer plus a row stride, the batch stride is T * ld.
//
// One MFMA shape carries every product: D[32x32] += A B with both operands read as ROW fragments
// (lane (r, h) holds a k-slice of row r), so Q, K, V and dO are only ever read along their rows:
//   * scores are computed transposed, S^T = K Q^T (A = K rows from LDS, B = the wave's Q rows held in
//     registers for the whole kernel).  A lane then owns ONE query and 16 of each 32 keys: the row
//     maximum and sum are in-lane reductions plus one v_permlane32_swap with the other half-wave.
//   * the exponentiated accumulator is the B operand of O^T += V^T P^T as it stands; the MFMA sums
//     over k in any order as long as A agrees, so V^T is read in the accumulator's key order:
//     bf16 by the transposing LDS read ds_read_b64_tr_b16 (rows 4h + {0..3} and + 8 of each 16 keys),
//     fp32 by plain ds_read_b32 (lane r reads column r of one key row: conflict free).
//   So K and V tiles lie in LDS row-major exactly as in memory, staged with 16-byte accesses; the
//   next tile's global loads are issued into registers before the current tile's MFMAs and written
//   to LDS after them (35 KB of LDS per block at DH = 128: two blocks fit a CU with room to spare).
// Forward: grid (ceil(Tq GS / 128), heads / GS, B), 4 waves of 32 queries; key tiles of 64 (bf16) or 32
//   (fp32) rows.  Online softmax in the exp2 domain (scale * log2 e folded into one multiply), the
//   O accumulators are rescaled only when some lane's running maximum moved, key tiles wholly above
//   the causal diagonal are skipped, tails and the diagonal are masked in the tile (-inf scores).
//   Epilogue: O / l rounded once, lse = m ln 2 + log l.
// Backward, two kernels, no atomics, nothing summed across blocks (deterministic):
//   dQ kernel, the forward's skeleton: P^T from lse, dP^T = V dO^T, dS^T = P^T (dP^T - delta) scale,
//     dQ^T += K^T dS^T; delta = rowsum(dO * O) from the wave's own register fragments.
//   dK/dV kernel, grid (ceil(Tk / 128), KV heads, B), a wave holds 32 keys' K and V rows in registers and
//     loops over staged query tiles (Q, dO, lse, and delta recomputed while dO and O are staged):
//     S = Q K^T, dP = dO V^T (a lane owns one key), dV^T += dO^T P, dK^T += Q^T dS.
//   The accumulate flag is applied in the final store (load, add in fp32, round once).
// fp32 storage runs the same kernels on v_mfma_f32_32x32x2_f32 with P and dS kept in fp32; its
// k-slices are the two halves of a row (lane half h holds columns h DH/2 ..), so fragments load as
// float4.  bf16 rounds P and dS to bf16 for the second product, the sums l stay fp32.
// Key lengths (klens, int32 [B], read on the device only; null: every key): key j of sample b takes part
//   iff j < klen = clamp(klens[b], 0, Tk).  klen replaces Tk wherever keys are bounded: the tile count (tiles
//   wholly past klen are never staged), the masks, and the rows a tile stages (padded rows are zeros in
//   LDS, their contents never meet an MFMA).  Query rows are never masked.  klen == 0 is the only way a
//   row can see no key: the forward stores output 0 and lse 0 for it, both backward kernels then visit no
//   key of that sample, so the row adds nothing to any gradient.  Padded key rows get dk = dv = 0 (left
//   alone under accumulate); a dK/dV lane of a padded key holds the fragments of the last visible key
//   instead of its own, so that its (select-zeroed) P and dS columns only ever multiply finite values.
// Grouped-query heads: k/v/dk/dv are [B, Tk, KH * DH], query head hd reads KV head hd / G, G = H / KH.
//   dK/dV: grid.y is the KV head, the block stages Q, dO, O and lse of the group's G query heads one
//   after the other inside the query-tile loop and sums them in one pair of register accumulators, in a
//   fixed order.  Forward and dQ: GS in {1, 2, 4} query heads of one group share a block (GS divides G):
//   wave w serves head GS blockIdx.y + w % GS and 32 of the block's 128 / GS query rows, so one staged
//   K/V tile feeds GS heads and K/V traffic falls GS-fold.  GS = 1 is the one-head block of plain MHA.
// Both are a template switch (EXT): without lengths and with G = 1 the dense instantiations run, which
//   hold none of this code.
// Supported: DH in {32, 64, 128}, any Tq, Tk >= 1, 16-byte aligned bases and row strides.
#include "common.h"

#include <initializer_list>

namespace {

typedef unsigned short bf16_t;
typedef __attribute__((address_space(3))) bf16x4_t lds_v4_t;

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> {
  static constexpr int KT = 64, PAD = 8, VE = 8;   // staged rows per tile, LDS row padding, elements per 16 B
};
template <> struct Cfg<float> {
  static constexpr int KT = 32, PAD = 4, VE = 4;
};

// row of the 32x32 accumulator held in register q of a lane in half h (the column is lane & 31)
FM_DEVICE int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// a = [a.lo | b.lo], b = [a.hi | b.hi] over the two 32-lane halves of the wave
FM_DEVICE float other_half(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return (threadIdx.x & 32) ? __uint_as_float(r[0]) : __uint_as_float(r[1]);
}

// ---- row fragments: every k-step operand of one DH-long row --------------------------------------
template <typename T, int DH> struct Frag;
template <int DH> struct Frag<bf16_t, DH> {
  bf16x8_t v[DH / 16];          // columns 16 ks + 8 h + e
};
template <int DH> struct Frag<float, DH> {
  float v[DH / 2];              // column h DH/2 + ks
};

template <int DH> FM_DEVICE void load_frag(Frag<bf16_t, DH>& f, const bf16_t* row, int h) {
#pragma unroll
  for (int ks = 0; ks < DH / 16; ++ks) f.v[ks] = *reinterpret_cast<const bf16x8_t*>(row + 16 * ks + 8 * h);
}
template <int DH> FM_DEVICE void load_frag(Frag<float, DH>& f, const float* row, int h) {
#pragma unroll
  for (int j = 0; j < DH / 8; ++j) {
    const f32x4_t t = *reinterpret_cast<const f32x4_t*>(row + h * (DH / 2) + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.v[4 * j + e] = t[e];
  }
}

// this lane's share of sum_c a[c] b[c]
template <int DH> FM_DEVICE float dot_frag(const Frag<bf16_t, DH>& a, const Frag<bf16_t, DH>& b) {
  float s = 0.f;
#pragma unroll
  for (int ks = 0; ks < DH / 16; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += bf2f((bf16_t)a.v[ks][e]) * bf2f((bf16_t)b.v[ks][e]);
  return s;
}
template <int DH> FM_DEVICE float dot_frag(const Frag<float, DH>& a, const Frag<float, DH>& b) {
  float s = 0.f;
#pragma unroll
  for (int ks = 0; ks < DH / 2; ++ks) s += a.v[ks] * b.v[ks];
  return s;
}

// ---- rotary position embedding ------------------------------------------------------------------------
// tab is fp32 [positions][DH]: row t holds cos(t w_i), i < DH/2, then sin(t w_i), computed on the host.  A row's
// column pairs (lo, hi) are (i, i + DH/2) (half-split) or (2i, 2i + 1) (inter, a wave-uniform runtime flag):
// lo' = lo c - hi s, hi' = hi c + lo s in fp32, rounded to storage once.  The transpose, which takes dq and dk
// back, is the same with -s.  Every access below is an aligned 8 or 16 bytes of one table row.
FM_DEVICE void rot(float& lo, float& hi, float c, float s) {
  const float x = lo * c - hi * s;
  hi = hi * c + lo * s;
  lo = x;
}
template <int N> FM_DEVICE void ldf(float (&d)[N], const float* __restrict__ p) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  if constexpr (N == 2) {
    const f32x2_t t = *reinterpret_cast<const f32x2_t*>(p);
    d[0] = t[0], d[1] = t[1];
  } else {
#pragma unroll
    for (int j = 0; j < N / 4; ++j) {
      const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[4 * j + e] = t[e];
    }
  }
}

// a register-resident row at position tr = tab + t DH.  bf16 holds both columns of a pair in one lane:
// v[ks] with v[ks + DH/32], or elements e, e + 1
template <int DH> FM_DEVICE void rope_frag(Frag<bf16_t, DH>& f, const float* __restrict__ tr, int inter, int h) {
  if (inter) {
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks) {                         // columns 16 ks + 8 h + e: frequencies 8 ks + 4 h + e / 2
      float c[4], s[4];
      ldf(c, tr + 8 * ks + 4 * h);
      ldf(s, tr + DH / 2 + 8 * ks + 4 * h);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float lo = bf2f((bf16_t)f.v[ks][2 * p]), hi = bf2f((bf16_t)f.v[ks][2 * p + 1]);
        rot(lo, hi, c[p], s[p]);
        f.v[ks][2 * p] = (short)f2bf(lo), f.v[ks][2 * p + 1] = (short)f2bf(hi);
      }
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < DH / 32; ++ks) {
      float c[8], s[8];
      ldf(c, tr + 16 * ks + 8 * h);
      ldf(s, tr + DH / 2 + 16 * ks + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float lo = bf2f((bf16_t)f.v[ks][e]), hi = bf2f((bf16_t)f.v[ks + DH / 32][e]);
        rot(lo, hi, c[e], s[e]);
        f.v[ks][e] = (short)f2bf(lo), f.v[ks + DH / 32][e] = (short)f2bf(hi);
      }
    }
  }
}
// fp32: lane half h holds column h DH/2 + ks, so an interleaved pair is (v[ks], v[ks + 1]) and the half-split
// partner of v[ks] is the other half-wave's v[ks] (half 0 holds lo, half 1 hi)
template <int DH> FM_DEVICE void rope_frag(Frag<float, DH>& f, const float* __restrict__ tr, int inter, int h) {
  if (inter) {
#pragma unroll
    for (int j = 0; j < DH / 8; ++j) {
      float c[2], s[2];
      ldf(c, tr + h * (DH / 4) + 2 * j);
      ldf(s, tr + DH / 2 + h * (DH / 4) + 2 * j);
      rot(f.v[4 * j], f.v[4 * j + 1], c[0], s[0]);
      rot(f.v[4 * j + 2], f.v[4 * j + 3], c[1], s[1]);
    }
  } else {
    const float sg = h ? 1.f : -1.f;
#pragma unroll
    for (int j = 0; j < DH / 8; ++j) {
      float c[4], s[4];
      ldf(c, tr + 4 * j);
      ldf(s, tr + DH / 2 + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) f.v[4 * j + e] = f.v[4 * j + e] * c[e] + sg * s[e] * other_half(f.v[4 * j + e]);
    }
  }
}

#define FM_ATTN_MFMA_BF16(a, b, c) \
  __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8v_t, a), __builtin_bit_cast(bf16x8v_t, b), c, 0, 0, 0)

// acc[i][c] += sum_k A[i][k] B[c][k]: A's row i = lane & 31 read from LDS at arow, B's row c in b
template <int DH> FM_DEVICE void mma_rows(f32x16_t& acc, const bf16_t* arow, const Frag<bf16_t, DH>& b, int h) {
#pragma unroll
  for (int ks = 0; ks < DH / 16; ++ks) {
    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(arow + 16 * ks + 8 * h);
    acc = FM_ATTN_MFMA_BF16(a, b.v[ks], acc);
  }
}
template <int DH> FM_DEVICE void mma_rows(f32x16_t& acc, const float* arow, const Frag<float, DH>& b, int h) {
#pragma unroll
  for (int j = 0; j < DH / 8; ++j) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(arow + h * (DH / 2) + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b.v[4 * j + e], acc, 0, 0, 0);
  }
}

// acc[nt][d][c] += sum_i X[i][32 nt + d] P[i][c] for the 32 rows i of the LDS tile x (row stride
// DH + PAD), P being a 32x32 accumulator: its registers are the B operand, X^T is read in their order
template <int DH> FM_DEVICE void mma_acc(f32x16_t (&acc)[DH / 32], const bf16_t* x, const f32x16_t& p, int lane) {
  constexpr int LD = DH + Cfg<bf16_t>::PAD;
  const int h = lane >> 5, g = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    bf16x8_t b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (short)f2bf(p[8 * u + e]);
    const bf16_t* a0 = x + (16 * u + 4 * h + q4) * LD + 16 * (g & 1) + 4 * p4;
#pragma unroll
    for (int nt = 0; nt < DH / 32; ++nt) {
      bf16x8_t a;
      a.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(a0 + 32 * nt));
      a.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(a0 + 8 * LD + 32 * nt));
      acc[nt] = FM_ATTN_MFMA_BF16(a, b, acc[nt]);
    }
  }
}
template <int DH> FM_DEVICE void mma_acc(f32x16_t (&acc)[DH / 32], const float* x, const f32x16_t& p, int lane) {
  constexpr int LD = DH + Cfg<float>::PAD;
  const int h = lane >> 5, r = lane & 31;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float* a0 = x + acc_row(q, h) * LD + r;
#pragma unroll
    for (int nt = 0; nt < DH / 32; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[32 * nt], p[q], acc[nt], 0, 0, 0);
  }
}

// ---- staging: NR rows x DH columns of a strided matrix through registers into a padded LDS tile ----
template <typename T, int DH, int NR> struct Stage {
  static constexpr int VE = Cfg<T>::VE, CPR = DH / VE, NCH = NR * CPR / 256, LD = DH + Cfg<T>::PAD;
  u32x4_t v[NCH];
  // rows >= nrows are zero in the tile (a masked P times zero, never times garbage)
  FM_DEVICE void load(const T* base, long ld, int row0, int nrows, int tid) {
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = tid + 256 * t, gr = row0 + c / CPR;
      v[t] = gr < nrows ? *reinterpret_cast<const u32x4_t*>(base + (long)gr * ld + (c % CPR) * VE) : u32x4_t{0u, 0u, 0u, 0u};
    }
  }
  // the loaded rows rotated on their way to LDS, row row0 + c / CPR at its own position.  An interleaved pair lies
  // inside a chunk, the half-split partner chunk is CPR / 2 lanes away in the same wave.  Rows >= nrows (>= 1) are
  // zeros and stay zeros: they read the last row of the table, the rotation of zeros is zero.
  FM_DEVICE void rope(const float* __restrict__ tab, int row0, int nrows, int tid, int inter) {
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = tid + 256 * t, col = (c % CPR) * VE;
      const float* tr = tab + (long)min(row0 + c / CPR, nrows - 1) * DH;
      float x[VE];
      unpack(x, v[t]);
      if (inter) {
        float cs[VE / 2], sn[VE / 2];
        ldf(cs, tr + col / 2);
        ldf(sn, tr + DH / 2 + col / 2);
#pragma unroll
        for (int p = 0; p < VE / 2; ++p) rot(x[2 * p], x[2 * p + 1], cs[p], sn[p]);
      } else {
        u32x4_t pv;
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = __shfl_xor(v[t][e], CPR / 2, 64);
        const float sg = col < DH / 2 ? -1.f : 1.f;
        float y[VE], cs[VE], sn[VE];
        unpack(y, pv);
        ldf(cs, tr + col % (DH / 2));
        ldf(sn, tr + DH / 2 + col % (DH / 2));
#pragma unroll
        for (int e = 0; e < VE; ++e) x[e] = x[e] * cs[e] + sg * sn[e] * y[e];
      }
      v[t] = pack(x);
    }
  }
  static FM_DEVICE void unpack(float (&x)[VE], const u32x4_t& a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (VE == 8) x[2 * e] = __uint_as_float(a[e] << 16), x[2 * e + 1] = __uint_as_float(a[e] & 0xffff0000u);
      else x[e] = __uint_as_float(a[e]);
    }
  }
  static FM_DEVICE u32x4_t pack(const float (&x)[VE]) {
    u32x4_t a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (VE == 8) a[e] = (unsigned)f2bf(x[2 * e]) | ((unsigned)f2bf(x[2 * e + 1]) << 16);
      else a[e] = __float_as_uint(x[e]);
    }
    return a;
  }
  FM_DEVICE void store(T* tile, int tid) const {
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int c = tid + 256 * t;
      *reinterpret_cast<u32x4_t*>(tile + (c / CPR) * LD + (c % CPR) * VE) = v[t];
    }
  }
};

FM_DEVICE float chunk_dot(const u32x4_t& a, const u32x4_t& b, bf16_t) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    s += __uint_as_float(a[e] << 16) * __uint_as_float(b[e] << 16) +
         __uint_as_float(a[e] & 0xffff0000u) * __uint_as_float(b[e] & 0xffff0000u);
  return s;
}
FM_DEVICE float chunk_dot(const u32x4_t& a, const u32x4_t& b, float) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) s += __uint_as_float(a[e]) * __uint_as_float(b[e]);
  return s;
}

// ---- the final store: 4 consecutive columns of one row, rounded once ------------------------------
FM_DEVICE void store4(bf16_t* p, f32x4_t v, bool add) {
  if (add) {
    const bf16x4_t o = *reinterpret_cast<const bf16x4_t*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += bf2f((bf16_t)o[e]);
  }
  bf16x4_t t;
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = (short)f2bf(v[e]);
  *reinterpret_cast<bf16x4_t*>(p) = t;
}
FM_DEVICE void store4(float* p, f32x4_t v, bool add) {
  if (add) v += *reinterpret_cast<const f32x4_t*>(p);
  *reinterpret_cast<f32x4_t*>(p) = v;
}

// the transposed accumulators acc[nt][d][row] of this lane's row to out[row][32 nt + d], times mul
template <typename T, int DH> FM_DEVICE void store_rows(const f32x16_t (&acc)[DH / 32], T* row, float mul, bool add, int h) {
#pragma unroll
  for (int nt = 0; nt < DH / 32; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4_t v = {acc[nt][4 * g] * mul, acc[nt][4 * g + 1] * mul, acc[nt][4 * g + 2] * mul, acc[nt][4 * g + 3] * mul};
      store4(row + 32 * nt + 8 * g + 4 * h, v, add);
    }
}

// dq / dk of the rotated rows taken back through the transpose of the rotation at tr, in the fp32 accumulators,
// before store_rows rounds them.  The lane holds columns 8 i + 4 h + e of its row in acc[i / 4][4 (i % 4) + e]:
// the half-split partner (+ DH/2) is i + DH/16 of the same lane, the interleaved one e ^ 1.
template <int DH> FM_DEVICE void unrope_acc(f32x16_t (&acc)[DH / 32], const float* __restrict__ tr, int inter, int h) {
  constexpr int NI = DH / 8;
  if (inter) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float c[2], s[2];
      ldf(c, tr + 4 * i + 2 * h);
      ldf(s, tr + DH / 2 + 4 * i + 2 * h);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float lo = acc[i / 4][4 * (i % 4) + 2 * p], hi = acc[i / 4][4 * (i % 4) + 2 * p + 1];
        rot(lo, hi, c[p], -s[p]);
        acc[i / 4][4 * (i % 4) + 2 * p] = lo, acc[i / 4][4 * (i % 4) + 2 * p + 1] = hi;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NI / 2; ++i) {
      constexpr int J = NI / 2;
      float c[4], s[4];
      ldf(c, tr + 8 * i + 4 * h);
      ldf(s, tr + DH / 2 + 8 * i + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float lo = acc[i / 4][4 * (i % 4) + e], hi = acc[(i + J) / 4][4 * ((i + J) % 4) + e];
        rot(lo, hi, c[e], -s[e]);
        acc[i / 4][4 * (i % 4) + e] = lo, acc[(i + J) / 4][4 * ((i + J) % 4) + e] = hi;
      }
    }
  }
}

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// the keys of sample b that take part (block-uniform)
FM_DEVICE int key_count(const int* __restrict__ klens, int b, int Tk) { return klens ? min(max(klens[b], 0), Tk) : Tk; }

// ---- forward ---------------------------------------------------------------------------------------
template <typename T, int DH, int GS, bool EXT, bool ROPE>
__global__ void __launch_bounds__(256) fm_attn_fwd(const T* __restrict__ q, long ldq, const T* __restrict__ k, long ldk,
                                                   const T* __restrict__ v, long ldv, T* __restrict__ o, long ldo,
                                                   float* __restrict__ lse, const int* __restrict__ klens,
                                                   const float* __restrict__ rope, int inter, int H, int G, int Tq, int Tk,
                                                   int causal, float sc2) {
  constexpr int KT = Cfg<T>::KT, LD = DH + Cfg<T>::PAD, NT = DH / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* ks = reinterpret_cast<T*>(smem);
  T* vs = ks + KT * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  constexpr int QB = 128 / GS;                                   // query rows of a block
  const int hd = blockIdx.y * GS + wave % GS, kvh = EXT ? blockIdx.y * GS / G : hd, b = blockIdx.z;
  const int klen = EXT ? key_count(klens, b, Tk) : Tk;
  q += (long)b * Tq * ldq + hd * DH;
  k += (long)b * Tk * ldk + kvh * DH;
  v += (long)b * Tk * ldv + kvh * DH;
  o += (long)b * Tq * ldo + hd * DH;
  const int q0 = blockIdx.x * QB + wave / GS * 32, qi = q0 + r;
  const bool active = q0 < Tq;                                   // wave-uniform
  Frag<T, DH> qf;
  load_frag(qf, q + (long)min(qi, Tq - 1) * ldq, h);
  if (ROPE) rope_frag(qf, rope + (long)min(qi, Tq - 1) * DH, inter, h);
  f32x16_t acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[nt][t] = 0.f;
  float m = -INFINITY, l = 0.f;                                  // l: this lane's keys only until the epilogue
  int nkt = (klen + KT - 1) / KT;
  if (causal) nkt = min(nkt, min(blockIdx.x * QB + QB - 1, Tq - 1) / KT + 1);
  Stage<T, DH, KT> sk, sv;
  sk.load(k, ldk, 0, klen, tid);
  sv.load(v, ldv, 0, klen, tid);
  for (int kt = 0; kt < nkt; ++kt) {
    if (ROPE) sk.rope(rope, kt * KT, klen, tid, inter);          // in registers, while the V loads are still in flight
    __syncthreads();                                             // the previous tile has been read
    sk.store(ks, tid);
    sv.store(vs, tid);
    __syncthreads();
    if (kt + 1 < nkt) {
      sk.load(k, ldk, (kt + 1) * KT, klen, tid);
      sv.load(v, ldv, (kt + 1) * KT, klen, tid);
    }
    const int k0 = kt * KT;
    if (!active || (causal && k0 > q0 + 31)) continue;           // wave-uniform
    f32x16_t s[KT / 32];
    const bool mask = k0 + KT > klen || (causal && k0 + KT - 1 > q0);
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < KT / 32; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[t][e] = 0.f;
      mma_rows<DH>(s[t], ks + (32 * t + r) * LD, qf, h);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float x = s[t][e] * sc2;
        if (mask) {
          const int key = k0 + 32 * t + acc_row(e, h);
          if (key >= klen || (causal && key > qi)) x = -INFINITY;
        }
        s[t][e] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = fmaxf(mx, other_half(mx));
    const float mn = fmaxf(m, mx);                               // finite: a tile is visited only if klen >= 1: key 0 is visible
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    if (__builtin_amdgcn_ballot_w64(mn > m) != 0) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] *= alpha;
    }
    l *= alpha;
    m = mn;
#pragma unroll
    for (int t = 0; t < KT / 32; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(s[t][e] - m);
        s[t][e] = p;
        l += p;
      }
      mma_acc<DH>(acc, vs + 32 * t * LD, s[t], lane);
    }
  }
  if (!active) return;
  l += other_half(l);
  if (qi < Tq) {
    // no visible key (klen == 0): output 0, and an lse the backward never uses (it visits no key either)
    const bool empty = EXT && l <= 0.f;
    store_rows<T, DH>(acc, o + (long)qi * ldo, empty ? 0.f : 1.f / l, false, h);
    if (h == 0) lse[((long)b * H + hd) * Tq + qi] = empty ? 0.f : m * LN2 + __logf(l);
  }
}

// ---- backward: dQ ------------------------------------------------------------------------------------
template <typename T, int DH, int GS, bool EXT, bool ROPE>
__global__ void __launch_bounds__(256) fm_attn_dq(const T* __restrict__ q, long ldq, const T* __restrict__ k, long ldk,
                                                  const T* __restrict__ v, long ldv, const T* __restrict__ o, long ldo,
                                                  const T* __restrict__ dout, long lddo, const float* __restrict__ lse,
                                                  T* __restrict__ dq, long lddq, int add, const int* __restrict__ klens,
                                                  const float* __restrict__ rope, int inter, int H, int G, int Tq, int Tk,
                                                  int causal, float scale) {
  constexpr int KT = Cfg<T>::KT, LD = DH + Cfg<T>::PAD, NT = DH / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* ks = reinterpret_cast<T*>(smem);
  T* vs = ks + KT * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  constexpr int QB = 128 / GS;                                   // query rows of a block
  const int hd = blockIdx.y * GS + wave % GS, kvh = EXT ? blockIdx.y * GS / G : hd, b = blockIdx.z;
  const int klen = EXT ? key_count(klens, b, Tk) : Tk;
  const float sc2 = scale * LOG2E;
  q += (long)b * Tq * ldq + hd * DH;
  k += (long)b * Tk * ldk + kvh * DH;
  v += (long)b * Tk * ldv + kvh * DH;
  o += (long)b * Tq * ldo + hd * DH;
  dout += (long)b * Tq * lddo + hd * DH;
  dq += (long)b * Tq * lddq + hd * DH;
  const int q0 = blockIdx.x * QB + wave / GS * 32, qi = q0 + r, qc = min(qi, Tq - 1);
  const bool active = q0 < Tq;
  Frag<T, DH> qf, dof;
  load_frag(qf, q + (long)qc * ldq, h);
  if (ROPE) rope_frag(qf, rope + (long)qc * DH, inter, h);
  load_frag(dof, dout + (long)qc * lddo, h);
  float delta;
  {
    Frag<T, DH> of;
    load_frag(of, o + (long)qc * ldo, h);
    delta = dot_frag(dof, of);
    delta += other_half(delta);
  }
  const float lse2 = lse[((long)b * H + hd) * Tq + qc] * LOG2E;
  f32x16_t acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[nt][t] = 0.f;
  int nkt = (klen + KT - 1) / KT;
  if (causal) nkt = min(nkt, min(blockIdx.x * QB + QB - 1, Tq - 1) / KT + 1);
  Stage<T, DH, KT> sk, sv;
  sk.load(k, ldk, 0, klen, tid);
  sv.load(v, ldv, 0, klen, tid);
  for (int kt = 0; kt < nkt; ++kt) {
    if (ROPE) sk.rope(rope, kt * KT, klen, tid, inter);
    __syncthreads();
    sk.store(ks, tid);
    sv.store(vs, tid);
    __syncthreads();
    if (kt + 1 < nkt) {
      sk.load(k, ldk, (kt + 1) * KT, klen, tid);
      sv.load(v, ldv, (kt + 1) * KT, klen, tid);
    }
    const int k0 = kt * KT;
    if (!active || (causal && k0 > q0 + 31)) continue;
#pragma unroll
    for (int t = 0; t < KT / 32; ++t) {
      f32x16_t s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      mma_rows<DH>(s, ks + (32 * t + r) * LD, qf, h);
      mma_rows<DH>(dp, vs + (32 * t + r) * LD, dof, h);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + 32 * t + acc_row(e, h);
        const float p = (key >= klen || (causal && key > qi)) ? 0.f : __builtin_amdgcn_exp2f(s[e] * sc2 - lse2);
        s[e] = p * (dp[e] - delta) * scale;
      }
      mma_acc<DH>(acc, ks + 32 * t * LD, s, lane);
    }
  }
  if (active && qi < Tq) {
    if (ROPE) unrope_acc<DH>(acc, rope + (long)qi * DH, inter, h);
    store_rows<T, DH>(acc, dq + (long)qi * lddq, 1.f, add != 0, h);
  }
}

// ---- backward: dK and dV -------------------------------------------------------------------------------
template <typename T, int DH, bool EXT, bool ROPE>
__global__ void __launch_bounds__(256) fm_attn_dkv(const T* __restrict__ q, long ldq, const T* __restrict__ k, long ldk,
                                                   const T* __restrict__ v, long ldv, const T* __restrict__ o, long ldo,
                                                   const T* __restrict__ dout, long lddo, const float* __restrict__ lse,
                                                   T* __restrict__ dk, long lddk, T* __restrict__ dv, long lddv, int addk,
                                                   int addv, const int* __restrict__ klens, const float* __restrict__ rope,
                                                   int inter, int H, int Gq, int Tq, int Tk, int causal, float scale) {
  constexpr int QT = Cfg<T>::KT, LD = DH + Cfg<T>::PAD, NT = DH / 32;
  typedef Stage<T, DH, QT> St;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* qs = reinterpret_cast<T*>(smem);
  T* dos = qs + QT * LD;
  float* lses = reinterpret_cast<float*>(dos + QT * LD);
  float* dels = lses + QT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int kvh = blockIdx.y, b = blockIdx.z;                    // the group's query heads: kvh G .. kvh G + G - 1
  const int G = EXT ? Gq : 1, klen = EXT ? key_count(klens, b, Tk) : Tk;
  // consecutive blocks go to different dies of the chip whatever their cost: with lengths the key blocks of a
  // (sample, head) are rotated by sample + head, so that no die gets the low, mostly live, key blocks only
  const int kb = EXT ? (blockIdx.x + kvh + b) % gridDim.x : blockIdx.x;
  const float sc2 = scale * LOG2E;
  q += (long)b * Tq * ldq + kvh * G * DH;
  k += (long)b * Tk * ldk + kvh * DH;
  v += (long)b * Tk * ldv + kvh * DH;
  o += (long)b * Tq * ldo + kvh * G * DH;
  dout += (long)b * Tq * lddo + kvh * G * DH;
  lse += ((long)b * H + kvh * G) * Tq;
  const int key0 = kb * 128 + wave * 32, kj = key0 + r;
  const bool active = key0 < klen;
  // a lane past klen takes the last visible key's rows: finite operands under its zeroed P and dS columns
  const int kc = EXT ? max(min(kj, klen - 1), 0) : min(kj, Tk - 1);
  Frag<T, DH> kf, vf;
  load_frag(kf, k + (long)kc * ldk, h);
  if (ROPE) rope_frag(kf, rope + (long)kc * DH, inter, h);       // the position of the row loaded
  load_frag(vf, v + (long)kc * ldv, h);
  f32x16_t acck[NT], accv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int t = 0; t < 16; ++t) acck[nt][t] = accv[nt][t] = 0.f;
  const int nqt = EXT && kb * 128 >= klen ? 0 : (Tq + QT - 1) / QT;   // a block wholly past klen stages nothing
  const int qt0 = causal ? kb * 128 / QT : 0;
  for (int qt = qt0, gi = 0; qt < nqt; ++gi == G ? (gi = 0, ++qt) : 0) {   // per query tile the group's heads in order
    const int qb = qt * QT;
    St sq, sd, so;
    sq.load(q + gi * DH, ldq, qb, Tq, tid);
    sd.load(dout + gi * DH, lddo, qb, Tq, tid);
    so.load(o + gi * DH, ldo, qb, Tq, tid);
    __syncthreads();                                             // the previous tile has been read
    if (!ROPE) sq.store(qs, tid);
    sd.store(dos, tid);
    // delta of a row: its St::CPR chunks sit in consecutive lanes
#pragma unroll
    for (int t = 0; t < St::NCH; ++t) {
      float d = chunk_dot(sd.v[t], so.v[t], T());
#pragma unroll
      for (int off = St::CPR / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
      const int c = tid + 256 * t;
      if (c % St::CPR == 0) dels[c / St::CPR] = d;
    }
    if (ROPE) {                                                  // once dO and O are done with, in their registers
      sq.rope(rope, qb, Tq, tid, inter);
      sq.store(qs, tid);
    }
    if (tid < QT) lses[tid] = qb + tid < Tq ? (EXT ? lse + (long)gi * Tq : lse)[qb + tid] * LOG2E : 0.f;
    __syncthreads();
    if (!active || (causal && qb + QT - 1 < key0)) continue;     // wave-uniform
#pragma unroll
    for (int t = 0; t < QT / 32; ++t) {
      f32x16_t s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
      mma_rows<DH>(s, qs + (32 * t + r) * LD, kf, h);
      mma_rows<DH>(dp, dos + (32 * t + r) * LD, vf, h);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = 32 * t + acc_row(e, h), qi = qb + i;
        const float p = (qi >= Tq || kj >= klen || (causal && kj > qi)) ? 0.f : __builtin_amdgcn_exp2f(s[e] * sc2 - lses[i]);
        s[e] = p;
        dp[e] = p * (dp[e] - dels[i]) * scale;
      }
      mma_acc<DH>(accv, dos + 32 * t * LD, s, lane);
      mma_acc<DH>(acck, qs + 32 * t * LD, dp, lane);
    }
  }
  if (kj >= Tk || (!EXT && !active)) return;
  if (EXT && kj >= klen) {                                              // a padded key: zeros, or the old value under accumulate
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int t = 0; t < 16; ++t) acck[nt][t] = accv[nt][t] = 0.f;
    if (addk) dk = nullptr;
    if (addv) dv = nullptr;
  }
  if (!ROPE && dk != nullptr) store_rows<T, DH>(acck, dk + ((long)b * Tk + kj) * lddk + kvh * DH, 1.f, addk != 0, h);
  if (dv != nullptr) store_rows<T, DH>(accv, dv + ((long)b * Tk + kj) * lddv + kvh * DH, 1.f, addv != 0, h);
  if (ROPE && dk != nullptr) {                                   // after dv has left its registers: fp32 DH = 128 needs them
    unrope_acc<DH>(acck, rope + (long)kj * DH, inter, h);
    store_rows<T, DH>(acck, dk + ((long)b * Tk + kj) * lddk + kvh * DH, 1.f, addk != 0, h);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// qlds: row strides of the [*, H dh] operands, kvlds: of the [*, KH dh] ones
template <typename T> int attn_status(int B, int H, int KH, int dh, int Tq, int Tk, int causal,
                                      std::initializer_list<const void*> ptrs, std::initializer_list<long> qlds,
                                      std::initializer_list<long> kvlds) {
  if (dh != 32 && dh != 64 && dh != 128) return FM_ATTN_HEAD_DIM;
  if (B < 1 || H < 1 || Tq < 1 || Tk < 1 || B > 65535 || H > 65535 || (causal && Tq != Tk)) return FM_ATTN_SHAPE;
  if (KH < 1 || H % KH != 0) return FM_ATTN_SHAPE;
  for (const void* p : ptrs)
    if (!al16(p)) return FM_ATTN_ALIGN;
  for (long ld : qlds)
    if (ld % Cfg<T>::VE != 0 || ld < (long)H * dh) return FM_ATTN_ALIGN;
  for (long ld : kvlds)
    if (ld % Cfg<T>::VE != 0 || ld < (long)KH * dh) return FM_ATTN_ALIGN;
  return 0;
}

template <typename T> size_t attn_lds(int dh) { return (size_t)2 * Cfg<T>::KT * (dh + Cfg<T>::PAD) * sizeof(T); }

// query heads of one group that share a forward / dQ block: the largest of 4, 2, 1 dividing G
int group_share(int G) { return G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1; }

// EXT: lengths or grouped heads, ROPE: a rotary table; the dense instantiations (both false, GS 1) carry none of that code
template <typename T, int GS, bool EXT, bool ROPE>
void launch_fwd(const T* q, long ldq, const T* k, long ldk, const T* v, long ldv, T* o, long ldo, float* lse,
                const int* klens, const float* rope, int inter, int B, int H, int G, int dh, int Tq, int Tk, int causal,
                float scale, hipStream_t s) {
  auto kern = dh == 32   ? fm_attn_fwd<T, 32, GS, EXT, ROPE>
              : dh == 64 ? fm_attn_fwd<T, 64, GS, EXT, ROPE>
                         : fm_attn_fwd<T, 128, GS, EXT, ROPE>;
  hipLaunchKernelGGL(kern, dim3((Tq * GS + 127) / 128, H / GS, B), dim3(256), attn_lds<T>(dh), s, q, ldq, k, ldk, v, ldv, o,
                     ldo, lse, klens, rope, inter, H, G, Tq, Tk, causal, scale * LOG2E);
}

template <typename T, int GS, bool EXT, bool ROPE>
void launch_dq(const T* q, long ldq, const T* k, long ldk, const T* v, long ldv, const T* o, long ldo, const T* dout,
               long lddo, const float* lse, T* dq, long lddq, int add, const int* klens, const float* rope, int inter, int B,
               int H, int G, int dh, int Tq, int Tk, int causal, float scale, hipStream_t s) {
  auto kern = dh == 32   ? fm_attn_dq<T, 32, GS, EXT, ROPE>
              : dh == 64 ? fm_attn_dq<T, 64, GS, EXT, ROPE>
                         : fm_attn_dq<T, 128, GS, EXT, ROPE>;
  hipLaunchKernelGGL(kern, dim3((Tq * GS + 127) / 128, H / GS, B), dim3(256), attn_lds<T>(dh), s, q, ldq, k, ldk, v, ldv, o,
                     ldo, dout, lddo, lse, dq, lddq, add, klens, rope, inter, H, G, Tq, Tk, causal, scale);
}

template <typename T, bool EXT, bool ROPE>
void launch_dkv(const T* q, long ldq, const T* k, long ldk, const T* v, long ldv, const T* o, long ldo, const T* dout,
                long lddo, const float* lse, T* dk, long lddk, T* dv, long lddv, int addk, int addv, const int* klens,
                const float* rope, int inter, int B, int H, int KH, int dh, int Tq, int Tk, int causal, float scale,
                hipStream_t s) {
  auto kern = dh == 32 ? fm_attn_dkv<T, 32, EXT, ROPE> : dh == 64 ? fm_attn_dkv<T, 64, EXT, ROPE> : fm_attn_dkv<T, 128, EXT, ROPE>;
  hipLaunchKernelGGL(kern, dim3((Tk + 127) / 128, KH, B), dim3(256), attn_lds<T>(dh) + 2 * Cfg<T>::KT * sizeof(float), s, q,
                     ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, dk, lddk, dv, lddv, addk, addv, klens, rope, inter, H,
                     H / KH, Tq, Tk, causal, scale);
}

// the instantiation a problem runs: lengths or grouped heads (ext) pick the block sharing gs
template <typename T, bool ROPE> auto pick_fwd(bool ext, int gs) {
  return !ext      ? launch_fwd<T, 1, false, ROPE>
         : gs == 4 ? launch_fwd<T, 4, true, ROPE>
         : gs == 2 ? launch_fwd<T, 2, true, ROPE>
                   : launch_fwd<T, 1, true, ROPE>;
}
template <typename T, bool ROPE> auto pick_dq(bool ext, int gs) {
  return !ext      ? launch_dq<T, 1, false, ROPE>
         : gs == 4 ? launch_dq<T, 4, true, ROPE>
         : gs == 2 ? launch_dq<T, 2, true, ROPE>
                   : launch_dq<T, 1, true, ROPE>;
}

template <typename T>
int attn_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo, float* lse, int B,
             int H, int KH, int dh, int Tq, int Tk, const int* klens, int causal, float scale, const float* rope, int inter,
             hipStream_t s) {
  if (int st = attn_status<T>(B, H, KH, dh, Tq, Tk, causal, {q, k, v, o, rope}, {ldq, ldo}, {ldk, ldv})) return st;
  const int G = H / KH, gs = group_share(G);
  const bool ext = klens != nullptr || G > 1;
  auto run = rope ? pick_fwd<T, true>(ext, gs) : pick_fwd<T, false>(ext, gs);
  run((const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (T*)o, ldo, lse, klens, rope, inter, B, H, G, dh, Tq, Tk, causal,
      scale, s);
  return 0;
}

template <typename T>
int attn_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* o, long ldo,
             const void* dout, long lddo, const float* lse, void* dq, long lddq, void* dk, long lddk, void* dv, long lddv,
             int acc_mask, int B, int H, int KH, int dh, int Tq, int Tk, const int* klens, int causal, float scale,
             const float* rope, int inter, hipStream_t s) {
  const long need = (long)H * dh;    // a gradient that is absent has no stride to check
  if (int st = attn_status<T>(B, H, KH, dh, Tq, Tk, causal, {q, k, v, o, dout, dq, dk, dv, rope},
                              {ldq, ldo, lddo, dq ? lddq : need}, {ldk, ldv, dk ? lddk : need, dv ? lddv : need}))
    return st;
  const int G = H / KH, gs = group_share(G);
  const bool ext = klens != nullptr || G > 1;
  if (dq != nullptr) {
    auto run = rope ? pick_dq<T, true>(ext, gs) : pick_dq<T, false>(ext, gs);
    run((const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (const T*)o, ldo, (const T*)dout, lddo, lse, (T*)dq, lddq,
        acc_mask & 1, klens, rope, inter, B, H, G, dh, Tq, Tk, causal, scale, s);
  }
  if (dk != nullptr || dv != nullptr) {
    auto run = rope ? (ext ? launch_dkv<T, true, true> : launch_dkv<T, false, true>)
                    : (ext ? launch_dkv<T, true, false> : launch_dkv<T, false, false>);
    run((const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (const T*)o, ldo, (const T*)dout, lddo, lse, (T*)dk, lddk,
        (T*)dv, lddv, (acc_mask >> 1) & 1, (acc_mask >> 2) & 1, klens, rope, inter, B, H, KH, dh, Tq, Tk, causal, scale, s);
  }
  return 0;
}

}  // namespace

extern "C" void fm_attention_error(int status, const char** msg) {
  *msg = status == 0                  ? "ok"
         : status == FM_ATTN_HEAD_DIM ? "attention: head dimension 32, 64 or 128"
         : status == FM_ATTN_SHAPE    ? "attention: 1..65535 samples and heads, Tq, Tk >= 1, causal needs Tq == Tk, kv_heads "
                                        "must divide heads"
         : status == FM_ATTN_ALIGN    ? "attention: 16-byte aligned bases and row strides (ld % 8 for bf16, ld % 4 for "
                                        "fp32), row strides of at least heads * dh (kv_heads * dh for k, v, dk, dv)"
                                      : "attention: unknown status";
}

extern "C" int fm_attention_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* o, long ldo,
                                float* lse, int B, int H, int KH, int dh, int Tq, int Tk, const int* key_lengths, int causal,
                                float scale, const float* rope, int rope_interleaved, hipStream_t s) {
  return attn_fwd<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, lse, B, H, KH, dh, Tq, Tk, key_lengths, causal, scale, rope,
                          rope_interleaved, s);
}

extern "C" int fm_attention_fwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o,
                                    long ldo, float* lse, int B, int H, int KH, int dh, int Tq, int Tk,
                                    const int* key_lengths, int causal, float scale, const float* rope,
                                    int rope_interleaved, hipStream_t s) {
  return attn_fwd<float>(q, ldq, k, ldk, v, ldv, o, ldo, lse, B, H, KH, dh, Tq, Tk, key_lengths, causal, scale, rope,
                         rope_interleaved, s);
}

extern "C" int fm_attention_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const void* o,
                                long ldo, const void* dout, long lddo, const float* lse, void* dq, long lddq, void* dk,
                                long lddk, void* dv, long lddv, int acc_mask, int B, int H, int KH, int dh, int Tq, int Tk,
                                const int* key_lengths, int causal, float scale, const float* rope, int rope_interleaved,
                                hipStream_t s) {
  return attn_bwd<bf16_t>(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, dq, lddq, dk, lddk, dv, lddv, acc_mask, B, H, KH,
                          dh, Tq, Tk, key_lengths, causal, scale, rope, rope_interleaved, s);
}

extern "C" int fm_attention_bwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                                    const float* o, long ldo, const float* dout, long lddo, const float* lse, float* dq,
                                    long lddq, float* dk, long lddk, float* dv, long lddv, int acc_mask, int B, int H, int KH,
                                    int dh, int Tq, int Tk, const int* key_lengths, int causal, float scale, const float* rope,
                                    int rope_interleaved, hipStream_t s) {
  return attn_bwd<float>(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, dq, lddq, dk, lddk, dv, lddv, acc_mask, B, H, KH,
                         dh, Tq, Tk, key_lengths, causal, scale, rope, rope_interleaved, s);
}
