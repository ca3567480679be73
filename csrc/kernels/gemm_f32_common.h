// Operand-side pieces of flexmi's fp32 MFMA GEMMs (gemm_f32.hip, gemm_x3.hip): the F16 form's scales,
// LDS image helpers, operand staging and fragment loads.  The parameter block GemmF, the output rule and
// the epilogues are gemm_epilogue.h's.  Internal linkage: every translation unit gets its own copy.
#pragma once
#include "gemm_epilogue.h"

namespace {

constexpr int NTF = 256;   // threads per block
constexpr int BKF = 32;    // k per LDS tile (fp32)

// the max over the np partials of index i (stride n)
FM_DEVICE unsigned amax_of(const unsigned* a, int np, int n, int i) {
  unsigned v = a[i];
  for (int k = 1; k < np; ++k) v = max(v, a[(long)k * n + i]);
  return v;
}

// power-of-two scale of a row / column whose max |x| has bit pattern mb: 2^sig with
// max * 2^sig in [2^14, 2^15) (an fp16 holds it with 11 significant bits and no overflow; a subnormal
// max counts by its leading bit); an all-zero row takes sig 0.  sig is clamped to the normal fp32
// exponent range, so rows below 2^-112 keep fp16 subnormal precision only (as fp32 itself does there).
FM_DEVICE int f16_sig(unsigned mb) {
  if (mb == 0) return 0;
  const int e = (int)(mb >> 23);
  const int eu = e ? e - 127 : (31 - __clz(mb)) - 149;
  const int sg = 14 - eu;
  return sg > 126 ? 126 : (sg < -126 ? -126 : sg);
}
FM_DEVICE float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }   // e in [-126, 127]

template <int N>
using fvec = float __attribute__((ext_vector_type(N)));

// byte offset of 16-B chunk c (4 floats) of row r in a K-contiguous image (128-B rows)
FM_DEVICE int kc_off(int r, int c) { return r * (BKF * 4) + 16 * (c ^ ((r >> 1) & 7)); }

// ---- global -> registers -> LDS (one operand tile) ----------------------------------------
template <bool KC, int R, bool VEC, int NT = NTF>
struct StageF {
  static constexpr int CHUNKS = R * BKF / 4;
  static constexpr int PER_T = CHUNKS / NT;
  static_assert(PER_T >= 1 && CHUNKS % NT == 0, "tile too small for the block");
  f32x4_t v[PER_T];

  FM_DEVICE void load(const float* __restrict__ p, long ld, int row0, int rows, int k0, int K, int tid) {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + NT * i;
      int gr, gk;
      if constexpr (KC) {
        gr = row0 + (ci >> 3);
        gk = k0 + 4 * (ci & 7);
      } else {
        gk = k0 + ci / (R / 4);
        gr = row0 + 4 * (ci % (R / 4));
      }
      if constexpr (VEC) {
        if (gr < rows && gk < K) {
          const float* src = KC ? (p + (long)gr * ld + gk) : (p + (long)gk * ld + gr);
          v[i] = *reinterpret_cast<const f32x4_t*>(src);
        } else {
          v[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rr = KC ? gr : gr + j;
          const int kk = KC ? gk + j : gk;
          v[i][j] = (rr < rows && kk < K) ? (KC ? p[(long)rr * ld + kk] : p[(long)kk * ld + rr]) : 0.f;
        }
      }
    }
  }

  FM_DEVICE void store(char* lds, int tid) {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + NT * i;
      int off;
      if constexpr (KC) off = kc_off(ci >> 3, ci & 7);
      else off = (ci / (R / 4)) * (R * 4) + 16 * (ci % (R / 4));
      *reinterpret_cast<f32x4_t*>(lds + off) = v[i];
    }
  }

  // MN-contiguous operand: every chunk of this thread covers the same 4 rows (tid % (R/4)),
  // so per-thread sums over the staged k are row partial sums (bias grad inside the dW GEMM)
  FM_DEVICE void accumulate_rows(float (&s)[4]) const {
#pragma unroll
    for (int i = 0; i < PER_T; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += v[i][j];
  }
};

// global -> LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, lane L's 16 B at
// base + 16 L): each lane loads the chunk the image layout (kc_off swizzle / linear MN rows) puts at
// its slot.  Full tiles only (the caller guarantees M, N multiples of the tile and K of BKF).
template <bool KC, int R, int NT>
struct DmaStageF {
  static constexpr int BYTES = R * BKF * 4;
  static constexpr int PER_W = BYTES / 1024 / (NT / 64);
  static_assert(PER_W >= 1 && BYTES % (1024 * (NT / 64)) == 0, "whole 1-KiB pieces per wave");
  FM_DEVICE static void issue(const float* __restrict__ p, long ld, int row0, int k0, char* lds, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_W; ++i) {
      const int piece = wave * PER_W + i;
      const int o = piece * 1024 + 16 * lane;
      const float* src;
      if constexpr (KC) {
        const int row = o / (BKF * 4), slot = (o % (BKF * 4)) / 16;
        src = p + (long)(row0 + row) * ld + k0 + 4 * (slot ^ ((row >> 1) & 7));
      } else {
        const int kr = o / (R * 4), ch = (o % (R * 4)) / 16;
        src = p + (long)(k0 + kr) * ld + row0 + 4 * ch;
      }
      __builtin_amdgcn_global_load_lds((gptr_t)(const void*)src, (lptr_t)(void*)(lds + piece * 1024), 16, 0, 0);
    }
  }
};

// fragments of one operand for one 16-wide k-chunk: f[t][s] = element (tile t, k-step s)
template <bool KC, int R, int T>
FM_DEVICE void load_frags(const char* lds, int base, int kk, int lane, float (&f)[T][4]) {
  const int q = lane & 15, g = lane >> 4;
  if constexpr (KC) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const f32x4_t x = *reinterpret_cast<const f32x4_t*>(lds + kc_off(base + 16 * t + q, 4 * kk + g));
#pragma unroll
      for (int s = 0; s < 4; ++s) f[t][s] = x[s];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 16 * kk + 4 * g + s;
      const fvec<T> x = *reinterpret_cast<const fvec<T>*>(lds + k * (R * 4) + 4 * (base + T * q));
#pragma unroll
      for (int t = 0; t < T; ++t) f[t][s] = x[t];
    }
  }
}

}  // namespace
