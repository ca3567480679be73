// Operand-side pieces shared by flexmi's MFMA kernels (gemm.hip, gemm_f32.hip / gemm_x3.hip, gemm_mp.h
// and the convolutions): bf16 LDS operand images + swizzles, MFMA fragment reads, the XCD-aware tile
// order and the in-order split-K slab sums.  The parameter blocks, the output rule and the epilogues
// built on it are in gemm_epilogue.h.
#pragma once
#include "common.h"

// LDS-DMA operand staging of the GEMM / convolution kernels is on (gemm_f32.hip: FM_GEMM_DMA, fm_gemm_set_dma)
extern "C" int fm_gemm_dma_enabled();

namespace {

constexpr int BK = 64;

typedef __attribute__((address_space(3))) bf16x4_t lds_v4_t;
// the operands of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// MN-contiguous operand image [k][R rows]: XOR swizzle of 16-B chunks per k-row so the
// transposing ds_read_b64_tr_b16 fragment reads of a 32-lane half hit every bank once.
template <int R>
struct MNSwz;
template <>
struct MNSwz<256> {  // 512-B rows, 32 chunks (same pattern as 128: stays inside 16-chunk halves)
  static FM_DEVICE int f(int k) { return 2 * ((k & 3) | (((k >> 3) & 1) << 2)); }
};
template <>
struct MNSwz<128> {  // 256-B rows, 16 chunks
  static FM_DEVICE int f(int k) { return 2 * ((k & 3) | (((k >> 3) & 1) << 2)); }
};
template <>
struct MNSwz<64> {  // 128-B rows, 8 chunks
  static FM_DEVICE int f(int k) { return 2 * (((k >> 1) & 1) | (((k >> 3) & 1) << 1)); }
};

// byte offset inside an operand LDS image.  K-contiguous image [row][64 k] (128-B rows, 16-B
// chunks XOR-swizzled by (row>>1)&7): conflict-free ds_read_b128 fragment reads.
template <bool KC, int R>
FM_DEVICE int lds_off(int row_or_k, int chunk) {
  if constexpr (KC) {
    return row_or_k * (BK * 2) + 16 * (chunk ^ ((row_or_k >> 1) & 7));
  } else {
    return row_or_k * (R * 2) + 16 * (chunk ^ MNSwz<R>::f(row_or_k));
  }
}

// ---- LDS -> MFMA fragment (8 bf16: k = 8*(lane>>4)+j for row/col lane&15) -------------
template <bool KC, int R>
FM_DEVICE bf16x8_t frag(const char* lds, int base, int kk, int lane) {
  if constexpr (KC) {
    int row = base + (lane & 15);
    int chunk = 4 * kk + (lane >> 4);
    return *reinterpret_cast<const bf16x8_t*>(lds + lds_off<true, R>(row, chunk));
  } else {
    int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    int chunk = (base >> 3) + (p >> 1);
    int k0 = 32 * kk + 8 * g + q;
    int o0 = lds_off<false, R>(k0, chunk) + 8 * (p & 1);
    int o1 = lds_off<false, R>(k0 + 4, chunk) + 8 * (p & 1);
    bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(lds + o0));
    bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t*)(lds + o1));
    bf16x8_t r;
    r.lo = lo;
    r.hi = hi;
    return r;
  }
}

// Sum of ks split-K slabs (MN floats apart) in slab order, with up to eight loads in flight: a
// plain `for k: s += slab[k]` waits for each load before issuing the next (one HBM round trip per
// slab -- 16 us for a 16-way reduce).  Same additions in the same order as that loop.
FM_DEVICE f32x4_t slab_sum4(const float* __restrict__ src, long MN, int ks) {
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= ks; k += 8) {
    f32x4_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4_t*>(src + (long)(k + u) * MN);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  if (k + 4 <= ks) {
    f32x4_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4_t*>(src + (long)(k + u) * MN);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += v[u];
    k += 4;
  }
  for (; k < ks; ++k) acc += *reinterpret_cast<const f32x4_t*>(src + (long)k * MN);
  return acc;
}
FM_DEVICE float slab_sum1(const float* __restrict__ src, long MN, int ks) {
  float acc = 0.f;
  int k = 0;
  for (; k + 8 <= ks; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(long)(k + u) * MN];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; k < ks; ++k) acc += src[(long)k * MN];
  return acc;
}

// XCD-aware bijective remap of the tile id (blocks b and b+8 share an XCD)
FM_DEVICE int xcd_remap(int bid, int ntiles) {
  int q = ntiles / 8, r = ntiles % 8, x = bid % 8;
  if (ntiles >= 8) bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
  return bid;
}

}  // namespace
