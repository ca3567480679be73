// LayerNorm / RMSNorm over the last dim with a fused residual add (Ba et al. 2016; Zhang & Sennrich 2019):
//   s = x (+ r)  formed in fp32, never rounded to the storage type
//   LayerNorm: y = (s - mean_D s) * rsqrt(var_D s + eps) * gamma + beta     (biased variance)
//   RMSNorm  : y = s * rsqrt(mean_D s^2 + eps) * gamma
// A pure streaming op, O(1) flops per byte: no matrix instruction has anything to do here, and the
// column sums of the backward ride along in registers.  One design for bf16 and fp32, both norms,
// with and without residual and affine weights:
//   * operands are base + row stride (elements), unit column stride: column slices of wider buffers
//     work, and nothing outside [row, 0..D) is written;
//   * the row lives in registers, every operand is read from memory once per pass.  A group of
//     G in {8, 16, 32, 64} lanes owns a row (256 / G rows per 256-thread block); G = 256 gives the
//     row to the whole block, whose four waves combine through LDS.  Lane l holds NV vectors of
//     V = 16 B / sizeof(T) elements at columns (l + k G) V, k < NV: one load instruction of a group
//     covers G * 16 contiguous bytes.  NV is a template constant, so the arrays stay in VGPRs;
//   * VEC = false is the same map with element accesses and a per-element mask: taken when D % V != 0
//     or a base or row stride is not 16-B aligned.  It is a switch on ldv / stv, not a second algorithm;
//   * statistics: in-lane sum, then a butterfly in the group (log2 G __shfl_xor steps); the variance is
//     the sum of (s - mean)^2 over the registers (two passes over registers, one over memory; the
//     one-pass E[s^2] - mean^2 cancels).  Masked columns contribute 0, the divisor is D.  fp32
//     (mean, rstd) per row is saved for the backward, rstd alone for RMSNorm;
//   * blocks are persistent over rows; a lane's columns never change, so it loads its gamma / beta
//     once, and in the backward keeps fp32 dgamma / dbeta partials for them across all its rows.
// Backward, two launches, no atomics (deterministic): the main kernel recomputes s, forms
//   g = dy * gamma,  ds = rstd * (g - mean_D g - xhat * mean_D(g * xhat))   (no mean_D g for RMSNorm)
// with the two row sums in one interleaved butterfly, stores dx and dresidual (each with its own
// accumulate flag, one rounding), folds the partials of the block's groups (same columns) through LDS
// in group order and writes one fp32 row [block, 2, D] to a workspace; the fold kernel sums those rows
// per column in a fixed order and adds into dgamma / dbeta.  Without affine weights (AFFINE = false)
// no partials are kept and the fold is not launched.
#include "common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_MAX_D = 8192;        // 256 lanes x 32 values
// Grid caps.  The forward has no per-block state in memory: 8 blocks per CU on 256 CUs, as fm_grid.
// The backward writes a [2, D] fp32 partial row per block, which the fold kernel reads again, so its
// grid is 4 blocks per CU for the lane groups (D <= 2048: at most 16 MiB of partials, and 16 waves per
// CU keep enough loads in flight) and 3 per CU for the block-per-row form (D <= 8192: at most 48 MiB).
// Three is what fits of its 16-values-per-lane instantiations (D <= 4096, 150 VGPRs; 2 per CU left bf16
// at 3.1 TB/s at 8192 x 3456); the 32-value ones (256 VGPRs) hold one block per CU, the rest queue.
constexpr int LN_FWD_CAP = 2048, LN_BWD_CAP = 1024, LN_BWD_CAP_BLOCK = 768;
constexpr int LN_FOLD_COLS = 32, LN_FOLD_SLICES = 32, LN_FOLD_THREADS = LN_FOLD_COLS * LN_FOLD_SLICES;

// ---- one vector of V columns starting at `col`; n = number of valid columns (0: absent row) -------
template <typename T, bool VEC, int V>
FM_DEVICE void ldv(const T* row, int col, int n, float (&v)[V]) {
  if (VEC) {
    if (col < n) {
      if constexpr (sizeof(T) == 2) {
        const bf16x8_t t = *reinterpret_cast<const bf16x8_t*>(row + col);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = bf2f((unsigned short)t[j]);
      } else {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(row + col);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = t[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = col + j < n ? ld<T>(row + col + j) : 0.f;
  }
}

template <typename T, bool VEC, int V>
FM_DEVICE void stv(T* row, int col, int n, const float (&v)[V]) {
  if (VEC) {
    if (col < n) {
      if constexpr (sizeof(T) == 2) {
        bf16x8_t t;
#pragma unroll
        for (int j = 0; j < V; ++j) t[j] = (short)f2bf(v[j]);
        *reinterpret_cast<bf16x8_t*>(row + col) = t;
      } else {
        *reinterpret_cast<f32x4_t*>(row + col) = f32x4_t{v[0], v[1], v[2], v[3]};
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (col + j < n) st<T>(row + col + j, v[j]);
  }
}

// V consecutive fp32 weights (gamma, beta); a null pointer gives `fill`
template <bool VEC, int V>
FM_DEVICE void ldw(const float* w, int col, int n, float fill, float (&v)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = fill;
  if (w == nullptr) return;
  if (VEC) {
    if (col < n) {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(w + col + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * q + j] = t[j];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (col + j < n) v[j] = w[col + j];
  }
}

// ---- sums over the G lanes of a row, every lane gets the result ------------------------------------
// G <= 64: butterfly inside the wave.  G = 256: the wave sums meet in LDS and are added in wave
// order; the leading barrier keeps a slow wave's reads of the previous call ahead of the writes.
template <int G>
FM_DEVICE void group_sum2(float& a, float& b, float (*red)[2]) {
  constexpr int W = G < 64 ? G : 64;
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) {   // the two sums interleaved: their shuffles overlap
    const float ta = __shfl_xor(a, o, 64), tb = __shfl_xor(b, o, 64);
    a += ta;
    b += tb;
  }
  if constexpr (G > 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][0] = a;
      red[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    b = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}
template <int G>
FM_DEVICE float group_sum(float a, float (*red)[2]) {
  float b = 0.f;
  group_sum2<G>(a, b, red);
  return a;
}

// s = x (+ r) for this lane's columns of one row
template <typename T, int G, int NV, bool VEC, int V>
FM_DEVICE void load_sum(const T* xr, const T* rr, int l, int n, float (&s)[NV][V]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int col = (l + k * G) * V;
    ldv<T, VEC, V>(xr, col, n, s[k]);
    if (rr) {
      float t[V];
      ldv<T, VEC, V>(rr, col, n, t);
#pragma unroll
      for (int j = 0; j < V; ++j) s[k][j] += t[j];
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------
// stats: [R, 2] (mean, rstd), or [R] rstd when rms
template <typename T, int G, int NV, bool VEC>
__global__ __launch_bounds__(LN_THREADS) void fm_layernorm_fwd(const T* __restrict__ x, long ldx, const T* __restrict__ r,
                                                               long ldr, T* __restrict__ y, long ldy,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ stats, long R, int D, float inv_d, float eps,
                                                               int rms) {
  constexpr int V = 16 / sizeof(T);
  constexpr int GPB = G <= 64 ? LN_THREADS / G : 1;   // rows per block
  __shared__ float red[4][2];
  const int l = threadIdx.x % G, grp = threadIdx.x / G;
  float gm[NV][V], bt[NV][V];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    ldw<VEC, V>(gamma, (l + k * G) * V, D, 1.f, gm[k]);
    ldw<VEC, V>(beta, (l + k * G) * V, D, 0.f, bt[k]);
  }
  // the trip count is one per block, so the shuffles and barriers below see whole waves
  for (long base = (long)blockIdx.x * GPB; base < R; base += (long)gridDim.x * GPB) {
    const long row = base + grp;
    const int n = row < R ? D : 0;
    float s[NV][V];
    load_sum<T, G, NV, VEC, V>(x + row * ldx, r ? r + row * ldr : nullptr, l, n, s);
    float mean = 0.f;
    if (!rms) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) a += s[k][j];
      mean = group_sum<G>(a, red) * inv_d;
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) s[k][j] = (l + k * G) * V + j < n ? s[k][j] - mean : 0.f;
    }
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) q += s[k][j] * s[k][j];
    const float rstd = rsqrtf(group_sum<G>(q, red) * inv_d + eps);
    if (l == 0 && n) {
      if (rms) {
        stats[row] = rstd;
      } else {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
      }
    }
    T* yr = y + row * ldy;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) s[k][j] = s[k][j] * rstd * gm[k][j] + bt[k][j];
      stv<T, VEC, V>(yr, (l + k * G) * V, n, s[k]);
    }
  }
}

// ---- backward, main kernel -------------------------------------------------------------------------
// The partials p of the block's groups, folded in group order into dst [D] (one row of the workspace)
template <int G, int NV, int V>
FM_DEVICE void fold_groups(const float (&p)[NV][V], float* part, float* __restrict__ dst, int l, int grp, int D) {
  if constexpr (G <= 64) {
    constexpr int E = G * NV * V, GPB = LN_THREADS / G;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) part[grp * E + (l + k * G) * V + j] = p[k][j];
    __syncthreads();
    for (int e = threadIdx.x; e < E && e < D; e += LN_THREADS) {
      float a = 0.f;
#pragma unroll
      for (int g = 0; g < GPB; ++g) a += part[g * E + e];
      dst[e] = a;
    }
  } else {   // one group: the lanes hold the block's sums already
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j)
        if ((l + k * G) * V + j < D) dst[(l + k * G) * V + j] = p[k][j];
  }
}

template <typename T, int G, int NV, bool VEC, bool AFFINE>
__global__ __launch_bounds__(LN_THREADS) void fm_layernorm_bwd(const T* __restrict__ x, long ldx, const T* __restrict__ r,
                                                               long ldr, const T* __restrict__ dy, long lddy,
                                                               const float* __restrict__ gamma, const float* __restrict__ stats,
                                                               T* __restrict__ dx, long lddx, T* __restrict__ dr, long lddr,
                                                               int accx, int accr, float* __restrict__ ws, long R, int D,
                                                               float inv_d, int rms) {
  constexpr int V = 16 / sizeof(T);
  constexpr int GPB = G <= 64 ? LN_THREADS / G : 1;
  constexpr int NW = AFFINE ? NV : 1;                 // no weight state without affine weights
  __shared__ float red[4][2];
  __shared__ float part[AFFINE && G <= 64 ? LN_THREADS * NV * V : 1];
  const int l = threadIdx.x % G, grp = threadIdx.x / G;
  float gm[NW][V], dg[NW][V], db[NW][V];
  if constexpr (AFFINE) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      ldw<VEC, V>(gamma, (l + k * G) * V, D, 1.f, gm[k]);
#pragma unroll
      for (int j = 0; j < V; ++j) dg[k][j] = db[k][j] = 0.f;
    }
  }
  for (long base = (long)blockIdx.x * GPB; base < R; base += (long)gridDim.x * GPB) {
    const long row = base + grp;
    const int n = row < R ? D : 0;
    float xh[NV][V], g[NV][V];
    load_sum<T, G, NV, VEC, V>(x + row * ldx, r ? r + row * ldr : nullptr, l, n, xh);
    const float mean = n && !rms ? stats[2 * row] : 0.f;
    const float rstd = n ? stats[rms ? row : 2 * row + 1] : 0.f;
    const T* dyr = dy + row * lddy;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      ldv<T, VEC, V>(dyr, (l + k * G) * V, n, g[k]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        xh[k][j] = (l + k * G) * V + j < n ? (xh[k][j] - mean) * rstd : 0.f;
        if constexpr (AFFINE) {
          dg[k][j] += g[k][j] * xh[k][j];
          db[k][j] += g[k][j];
          g[k][j] *= gm[k][j];
        }
        a += g[k][j];
        b += g[k][j] * xh[k][j];
      }
    }
    if (dx == nullptr && dr == nullptr) continue;   // weight gradients only (block-uniform)
    group_sum2<G>(a, b, red);
    a = rms ? 0.f : a * inv_d;
    b *= inv_d;
    T* dxr = dx ? dx + row * lddx : nullptr;
    T* drr = dr ? dr + row * lddr : nullptr;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int col = (l + k * G) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) g[k][j] = rstd * (g[k][j] - a - xh[k][j] * b);
      float o[V], t[V];
      if (dxr) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = g[k][j];
        if (accx) {
          ldv<T, VEC, V>(dxr, col, n, t);
#pragma unroll
          for (int j = 0; j < V; ++j) o[j] += t[j];
        }
        stv<T, VEC, V>(dxr, col, n, o);
      }
      if (drr) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = g[k][j];
        if (accr) {
          ldv<T, VEC, V>(drr, col, n, t);
#pragma unroll
          for (int j = 0; j < V; ++j) o[j] += t[j];
        }
        stv<T, VEC, V>(drr, col, n, o);
      }
    }
  }
  if constexpr (AFFINE) {
    float* out = ws + (long)blockIdx.x * 2 * D;
    fold_groups<G, NV, V>(dg, part, out, l, grp, D);
    if (!rms) fold_groups<G, NV, V>(db, part, out + D, l, grp, D);
  }
}

// ---- backward, fold kernel: dgamma / dbeta [D] += the sum over the blocks' partial rows -------------
// blockIdx.y picks dgamma or dbeta; a block of 1024 takes 32 columns, its 32 slices of lanes take every
// 32nd partial row, eight loads in flight at a time (the partials were written by other XCDs, so every
// load pays the way to memory: one at a time took 11 us for 32 of them), and meet in LDS in slice order.
__global__ __launch_bounds__(LN_FOLD_THREADS) void fm_layernorm_fold(const float* __restrict__ ws, int nblk, int D,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float part[LN_FOLD_SLICES][LN_FOLD_COLS];
  const int w = blockIdx.y, cx = threadIdx.x % LN_FOLD_COLS, sl = threadIdx.x / LN_FOLD_COLS;
  const int c = blockIdx.x * LN_FOLD_COLS + cx;
  float* dst = w ? dbeta : dgamma;
  float a = 0.f;
  if (c < D)
    for (int b0 = sl; b0 < nblk; b0 += 8 * LN_FOLD_SLICES) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + u * LN_FOLD_SLICES;
        v[u] = b < nblk ? ws[((long)b * 2 + w) * D + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
  part[sl][cx] = a;
  __syncthreads();
  if (sl == 0 && c < D) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < LN_FOLD_SLICES; ++i) t += part[i][cx];
    dst[c] += t;
  }
}

// ---- host ------------------------------------------------------------------------------------------
struct LnPlan {
  int G, vals;   // lanes per row (256: the block), values per lane (8, 16 or 32)
};

// The smallest group whose lanes hold 8 values each; past 64 lanes the lanes hold more, up to 32;
// past that the row takes the whole block.
LnPlan ln_plan(int D) {
  for (int G = 8; G <= 64; G *= 2)
    if (G * 8 >= D) return {G, 8};
  if (64 * 16 >= D) return {64, 16};
  if (64 * 32 >= D) return {64, 32};
  return {256, D <= 256 * 16 ? 16 : 32};
}

bool ln_al16(const void* p, long ld, size_t elem) { return (((uintptr_t)p) & 15) == 0 && (ld * (long)elem) % 16 == 0; }

int ln_bwd_grid(const LnPlan& p, long R) {
  const long rows = p.G <= 64 ? LN_THREADS / p.G : 1;
  const long want = (R + rows - 1) / rows, cap = p.G <= 64 ? LN_BWD_CAP : LN_BWD_CAP_BLOCK;
  return (int)(want < cap ? want : cap);
}

#define LN_PLANS(X) X(8, 8) X(16, 8) X(32, 8) X(64, 8) X(64, 16) X(64, 32) X(256, 16) X(256, 32)

template <typename T>
void ln_forward(const T* x, long ldx, const T* r, long ldr, T* y, long ldy, const float* gamma, const float* beta, float* stats,
                long R, int D, float eps, int rms, hipStream_t s) {
  constexpr int V = 16 / sizeof(T);
  const LnPlan p = ln_plan(D);
  const bool vec = D % V == 0 && ln_al16(x, ldx, sizeof(T)) && ln_al16(r, ldr, sizeof(T)) && ln_al16(y, ldy, sizeof(T)) &&
                   ln_al16(gamma, 0, 4) && ln_al16(beta, 0, 4);
  const long rows = p.G <= 64 ? LN_THREADS / p.G : 1, want = (R + rows - 1) / rows;
  const dim3 grid((unsigned)(want < LN_FWD_CAP ? want : LN_FWD_CAP));
#define X(G_, VALS_)                                                                                                      \
  if (p.G == G_ && p.vals == VALS_) {                                                                                     \
    if (vec)                                                                                                              \
      hipLaunchKernelGGL((fm_layernorm_fwd<T, G_, VALS_ / V, true>), grid, dim3(LN_THREADS), 0, s, x, ldx, r, ldr, y, ldy, \
                         gamma, beta, stats, R, D, 1.f / D, eps, rms);                                                    \
    else                                                                                                                  \
      hipLaunchKernelGGL((fm_layernorm_fwd<T, G_, VALS_ / V, false>), grid, dim3(LN_THREADS), 0, s, x, ldx, r, ldr, y, ldy, \
                         gamma, beta, stats, R, D, 1.f / D, eps, rms);                                                    \
  }
  LN_PLANS(X)
#undef X
}

template <typename T, bool AFFINE>
void ln_backward(const T* x, long ldx, const T* r, long ldr, const T* dy, long lddy, const float* gamma, const float* stats,
                 T* dx, long lddx, T* dr, long lddr, int accx, int accr, float* ws, int nblk, long R, int D, int rms,
                 hipStream_t s) {
  constexpr int V = 16 / sizeof(T);
  const LnPlan p = ln_plan(D);
  const bool vec = D % V == 0 && ln_al16(x, ldx, sizeof(T)) && ln_al16(r, ldr, sizeof(T)) && ln_al16(dy, lddy, sizeof(T)) &&
                   ln_al16(dx, lddx, sizeof(T)) && ln_al16(dr, lddr, sizeof(T)) && ln_al16(gamma, 0, 4);
  const dim3 grid((unsigned)nblk);
#define X(G_, VALS_)                                                                                                     \
  if (p.G == G_ && p.vals == VALS_) {                                                                                    \
    if (vec)                                                                                                             \
      hipLaunchKernelGGL((fm_layernorm_bwd<T, G_, VALS_ / V, true, AFFINE>), grid, dim3(LN_THREADS), 0, s, x, ldx, r, ldr, \
                         dy, lddy, gamma, stats, dx, lddx, dr, lddr, accx, accr, ws, R, D, 1.f / D, rms);                \
    else                                                                                                                 \
      hipLaunchKernelGGL((fm_layernorm_bwd<T, G_, VALS_ / V, false, AFFINE>), grid, dim3(LN_THREADS), 0, s, x, ldx, r, ldr, \
                         dy, lddy, gamma, stats, dx, lddx, dr, lddr, accx, accr, ws, R, D, 1.f / D, rms);                \
  }
  LN_PLANS(X)
#undef X
}

}  // namespace

extern "C" long fm_layernorm_ws_bytes(long R, int D) {
  if (D < 1 || D > LN_MAX_D || R <= 0) return 0;
  return (long)ln_bwd_grid(ln_plan(D), R) * 2 * D * (long)sizeof(float);
}

extern "C" int fm_layernorm_forward(const void* x, long ldx, const void* r, long ldr, void* y, long ldy,
                                    const float* gamma, const float* beta, float* stats, long R, int D, float eps,
                                    int rms, int bf16, hipStream_t s) {
  if (D < 1 || D > LN_MAX_D) return 1;
  if (R <= 0) return 0;
  if (rms) beta = nullptr;
  if (bf16)
    ln_forward<unsigned short>((const unsigned short*)x, ldx, (const unsigned short*)r, ldr, (unsigned short*)y, ldy, gamma, beta,
                               stats, R, D, eps, rms, s);
  else
    ln_forward<float>((const float*)x, ldx, (const float*)r, ldr, (float*)y, ldy, gamma, beta, stats, R, D, eps, rms, s);
  return 0;
}

extern "C" int fm_layernorm_backward(const void* x, long ldx, const void* r, long ldr, const void* dy, long lddy,
                                     const float* gamma, const float* stats, void* dx, long lddx, void* dr, long lddr,
                                     int accx, int accr, float* dgamma, float* dbeta, float* ws, long ws_bytes, long R,
                                     int D, int rms, int bf16, hipStream_t s) {
  if (D < 1 || D > LN_MAX_D) return 1;
  const bool affine = dgamma != nullptr;
  if (R <= 0 || (!dx && !dr && !affine)) return 0;
  if (affine && (ws == nullptr || ws_bytes < fm_layernorm_ws_bytes(R, D))) return 2;
  const int nblk = ln_bwd_grid(ln_plan(D), R);
#define LN_BWD(T_, AFF_)                                                                                                 \
  ln_backward<T_, AFF_>((const T_*)x, ldx, (const T_*)r, ldr, (const T_*)dy, lddy, gamma, stats, (T_*)dx, lddx, (T_*)dr, lddr, \
                        accx, accr, ws, nblk, R, D, rms, s)
  if (bf16) {
    if (affine) LN_BWD(unsigned short, true); else LN_BWD(unsigned short, false);
  } else {
    if (affine) LN_BWD(float, true); else LN_BWD(float, false);
  }
#undef LN_BWD
  if (affine) {
    const dim3 grid((D + LN_FOLD_COLS - 1) / LN_FOLD_COLS, rms || dbeta == nullptr ? 1 : 2);
    hipLaunchKernelGGL(fm_layernorm_fold, grid, dim3(LN_FOLD_THREADS), 0, s, (const float*)ws, nblk, D, dgamma, dbeta);
  }
  return 0;
}
