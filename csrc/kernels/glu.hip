// Gated feed-forward (SwiGLU / GeGLU) for gfx950 (MI355X / CDNA4).
//
//   gu[M, 2F] = x[M, H] W[2F, H]^T        rows [0, F) of W = gate, rows [F, 2F) = up
//   h[M, F]   = act(g) * u                g = gu[:, :F], u = gu[:, F:], act = SiLU or exact (erf) GELU
//
// fm_glu_gemm_fwd is the fused forward on bf16 operands: a block owns a 128 x 64 tile of h and computes
// the matching 128 x 64 tiles of g AND u from ONE staged x tile -- per 64-deep k step it stages x
// [128][64] and the two weight tiles [64][64] (rows n0.. and F + n0.. of W), together the LDS footprint
// of a 128 x 128 GEMM tile, as K-contiguous XOR-swizzled images (gemm_common.h), double-buffered.  Four
// waves in 2 x 2; a wave holds 64 rows x 32 columns of g and the same 64 x 32 of u in two accumulator
// sets (2 x 8 tiles of v_mfma_f32_16x16x32_bf16, 64 fp32 accumulators) and every x fragment read from
// LDS feeds both sets.  The MFMA operands are swapped as in gemm.hip, so a lane owns 4 consecutive
// columns of one row of g and of u: the epilogue rounds both to bf16, stores them into gu (columns c
// and F + c: the backward reads them), forms act(g) * u in fp32 FROM THE ROUNDED values and stores h --
// no pass over memory between the GEMM and h.  Full tiles stage by LDS-DMA (each lane loads the 16-B
// chunk the swizzle puts at its slot), every other legal shape by registers with zero-filled edge
// chunks and masked stores (template switch DMA).  Tile order is XCD-aware.
//
// fm_glu_act_fwd / fm_glu_act_bwd are the element-wise halves of the composed forward (a plain GEMM
// with N = 2F, then act_fwd) and of the backward:  dg = dh * u * act'(g), du = dh * act(g), written
// side by side into dgu [M, 2F] so that dX and dW are each ONE ordinary GEMM over K = 2F / N = 2F.
// 16-byte accesses, fp32 arithmetic, one rounding on store; an element path with a mask serves widths
// that are no multiple of the vector and misaligned operands.
#include "gemm_common.h"

#include <algorithm>

namespace {

enum { GLU_SILU = 0, GLU_GELU = 1 };

// sigma(g) and Phi(g): act(g) = g * gate(g)
FM_DEVICE float glu_sigmoid(float g) { return 1.f / (1.f + __expf(-g)); }
FM_DEVICE float glu_phi_cdf(float g) { return 0.5f * (1.f + erff(g * 0.70710678118654752f)); }

FM_DEVICE float glu_act(int act, float g) { return g * (act == GLU_SILU ? glu_sigmoid(g) : glu_phi_cdf(g)); }

// silu'(g) = s (1 + g (1 - s));  gelu'(g) = Phi(g) + g phi(g)
FM_DEVICE float glu_dact(int act, float g) {
  if (act == GLU_SILU) {
    const float s = glu_sigmoid(g);
    return s * (1.f + g * (1.f - s));
  }
  return glu_phi_cdf(g) + g * 0.39894228040143268f * __expf(-0.5f * g * g);
}

// ------------------------------------------------------------------------------------------------
// fused forward
constexpr int GNT = 256;                       // 4 waves, 2 x 2
constexpr int GBM = 128, GBN = 64;             // tile of h
constexpr int X_BYTES = GBM * BK * 2;          // 16 KiB
constexpr int W_BYTES = GBN * BK * 2;          // 8 KiB, twice (gate, up)
constexpr int STAGE_BYTES = X_BYTES + 2 * W_BYTES;

struct GluP {
  const unsigned short* x; long ldx;
  const unsigned short* w;                     // [2F][H], contiguous
  unsigned short* gu;                          // [M][2F], contiguous
  unsigned short* h; long ldh;
  int M, F, H, act;
  int tiles_m, tiles_n;
};

// global -> registers of one K-contiguous operand tile [R][64]: 16-B chunks, zero-filled past the edges
template <int R>
struct GluStage {
  static constexpr int PER_T = R * BK / 8 / GNT;
  u32x4_t v[PER_T];

  FM_DEVICE void load(const unsigned short* __restrict__ p, long ld, int row0, int rows, int k0, int K, int tid) {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + GNT * i;
      const int gr = row0 + (ci >> 3), gk = k0 + 8 * (ci & 7);
      // K % 8 == 0 (launcher): a chunk is wholly inside or wholly outside the row
      v[i] = (gr < rows && gk < K) ? *reinterpret_cast<const u32x4_t*>(p + (long)gr * ld + gk) : u32x4_t{0u, 0u, 0u, 0u};
    }
  }
  FM_DEVICE void store(char* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + GNT * i;
      *reinterpret_cast<u32x4_t*>(lds + lds_off<true, R>(ci >> 3, ci & 7)) = v[i];
    }
  }
};

// global -> LDS by LDS-DMA, full tiles only: one wave-instruction fills 1 KiB of the image, lane L's 16 B
// land at piece + 16 L, so the lane loads the chunk the swizzle puts there (the inverse of lds_off)
template <int R>
FM_DEVICE void glu_dma(const unsigned short* __restrict__ p, long ld, int row0, int k0, char* lds, int wave, int lane) {
  constexpr int PER_W = R * BK * 2 / 1024 / (GNT / 64);
  static_assert(PER_W >= 1, "whole 1-KiB pieces per wave");
#pragma unroll
  for (int i = 0; i < PER_W; ++i) {
    const int piece = wave * PER_W + i;
    const int o = piece * 1024 + 16 * lane;
    const int row = o / (BK * 2), slot = (o % (BK * 2)) / 16;
    const int c = slot ^ ((row >> 1) & 7);
    const unsigned short* src = p + (long)(row0 + row) * ld + k0 + 8 * c;
    __builtin_amdgcn_global_load_lds((gptr_t)(const void*)src, (lptr_t)(void*)(lds + piece * 1024), 16, 0, 0);
  }
}

template <bool DMA>
__global__ void __launch_bounds__(GNT, 2) fm_glu_gemm_kernel(GluP p) {
  constexpr int MR = 4, NR = 2;                // 16 x 16 subtiles of a wave: 64 rows x 32 columns
  extern __shared__ __attribute__((aligned(16))) char smem[];
#define LDS_X(b) (smem + (b) * STAGE_BYTES)
#define LDS_G(b) (smem + (b) * STAGE_BYTES + X_BYTES)
#define LDS_U(b) (smem + (b) * STAGE_BYTES + X_BYTES + W_BYTES)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware order; column tiles fastest, so the blocks of one XCD share an x row tile
  const int bid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
  const int m0 = (bid / p.tiles_n) * GBM, n0 = (bid % p.tiles_n) * GBN;

  const unsigned short* wg = p.w;
  const unsigned short* wu = p.w + (long)p.F * p.H;
  const int ktiles = (p.H + BK - 1) / BK;

  f32x4_t ag[MR][NR], au[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) ag[i][j] = au[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  GluStage<GBM> sx;
  GluStage<GBN> sg, su;
  auto stage_dma = [&](int kt, int b) {
    glu_dma<GBM>(p.x, p.ldx, m0, kt * BK, LDS_X(b), wave, lane);
    glu_dma<GBN>(wg, p.H, n0, kt * BK, LDS_G(b), wave, lane);
    glu_dma<GBN>(wu, p.H, n0, kt * BK, LDS_U(b), wave, lane);
  };
  auto stage_load = [&](int kt) {
    sx.load(p.x, p.ldx, m0, p.M, kt * BK, p.H, tid);
    sg.load(wg, p.H, n0, p.F, kt * BK, p.H, tid);
    su.load(wu, p.H, n0, p.F, kt * BK, p.H, tid);
  };
  auto stage_store = [&](int b) {
    sx.store(LDS_X(b), tid);
    sg.store(LDS_G(b), tid);
    su.store(LDS_U(b), tid);
  };
  if constexpr (DMA) {
    stage_dma(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  } else {
    stage_load(0);
    stage_store(0);
  }
  __syncthreads();

  for (int kt = 0; kt < ktiles; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < ktiles;
    if (more) {
      if constexpr (DMA) stage_dma(kt + 1, cur ^ 1);
      else stage_load(kt + 1);
    }
    const char* lx = LDS_X(cur);
    const char* lg = LDS_G(cur);
    const char* lu = LDS_U(cur);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8_t xf[MR], gf[NR], uf[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) xf[i] = frag<true, GBM>(lx, wm * 64 + 16 * i, kk, lane);
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        gf[j] = frag<true, GBN>(lg, wn * 32 + 16 * j, kk, lane);
        uf[j] = frag<true, GBN>(lu, wn * 32 + 16 * j, kk, lane);
      }
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          // operands swapped (weight fragment as the MFMA "A"): a lane owns 4 consecutive columns
          ag[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8v_t*>(&gf[j]),
                                                             *reinterpret_cast<bf16x8v_t*>(&xf[i]), ag[i][j], 0, 0, 0);
          au[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8v_t*>(&uf[j]),
                                                             *reinterpret_cast<bf16x8v_t*>(&xf[i]), au[i][j], 0, 0, 0);
        }
    }
    if constexpr (DMA) {
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's pieces of step kt + 1 landed
    } else if (more) {
      stage_store(cur ^ 1);
    }
    __syncthreads();
  }
#undef LDS_X
#undef LDS_G
#undef LDS_U

  // epilogue: lane (q, g4) holds g and u of row 16 i + q, columns 16 j + 4 g4 .. + 3 of the wave tile
  const int q = lane & 15, g4 = lane >> 4;
  const long ldgu = 2L * p.F;
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    const int m = m0 + wm * 64 + 16 * i + q;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int n = n0 + wn * 32 + 16 * j + 4 * g4;
      // F % 4 == 0 (launcher): a quad is wholly inside or wholly outside
      if (!DMA && (m >= p.M || n >= p.F)) continue;
      bf16x4_t gq, uq, hq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned short gb = f2bf(ag[i][j][r]), ub = f2bf(au[i][j][r]);
        gq[r] = (short)gb;
        uq[r] = (short)ub;
        hq[r] = (short)f2bf(glu_act(p.act, bf2f(gb)) * bf2f(ub));
      }
      unsigned short* gurow = p.gu + (long)m * ldgu + n;
      *reinterpret_cast<bf16x4_t*>(gurow) = gq;
      *reinterpret_cast<bf16x4_t*>(gurow + p.F) = uq;
      *reinterpret_cast<bf16x4_t*>(p.h + (long)m * p.ldh + n) = hq;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// element-wise halves: W elements per thread-step (16 B; 1 on the element path)
template <typename T> struct GluVec;
template <> struct GluVec<unsigned short> { static constexpr int W = 8; };
template <> struct GluVec<float> { static constexpr int W = 4; };

template <int W, typename T>
FM_DEVICE void glu_ld(const T* p, float (&v)[W]) {
  if constexpr (W == 8) {
    ld8<T>(p, v);
  } else if constexpr (W == 4) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j];
  } else {
    v[0] = ld<T>(p);
  }
}
template <int W, typename T>
FM_DEVICE void glu_st(T* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    st8<T>(p, v);
  } else if constexpr (W == 4) {
    *reinterpret_cast<f32x4_t*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
  } else {
    st<T>(p, v[0]);
  }
}

// h = act(g) * u.  A step is W consecutive columns of one row; cpr = F / W steps per row.
template <typename T, int W>
__global__ void __launch_bounds__(256) fm_glu_act_fwd_kernel(const T* __restrict__ gu, long ldgu, T* __restrict__ h, long ldh,
                                                            long M, int F, int act) {
  const long cpr = F / W, total = M * cpr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long m = idx / cpr;
    const int c = (int)(idx - m * cpr) * W;
    float g[W], u[W], o[W];
    glu_ld<W, T>(gu + m * ldgu + c, g);
    glu_ld<W, T>(gu + m * ldgu + F + c, u);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = glu_act(act, g[j]) * u[j];
    glu_st<W, T>(h + m * ldh + c, o);
  }
}

// dg = dh * u * act'(g), du = dh * act(g) into columns c and F + c of dgu
template <typename T, int W>
__global__ void __launch_bounds__(256) fm_glu_act_bwd_kernel(const T* __restrict__ dh, long lddh, const T* __restrict__ gu,
                                                            long ldgu, T* __restrict__ dgu, long lddgu, long M, int F,
                                                            int act) {
  const long cpr = F / W, total = M * cpr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long m = idx / cpr;
    const int c = (int)(idx - m * cpr) * W;
    float d[W], g[W], u[W], dg[W], du[W];
    glu_ld<W, T>(dh + m * lddh + c, d);
    glu_ld<W, T>(gu + m * ldgu + c, g);
    glu_ld<W, T>(gu + m * ldgu + F + c, u);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      dg[j] = d[j] * u[j] * glu_dact(act, g[j]);
      du[j] = d[j] * glu_act(act, g[j]);
    }
    glu_st<W, T>(dgu + m * lddgu + c, dg);
    glu_st<W, T>(dgu + m * lddgu + F + c, du);
  }
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <typename T>
void glu_act_fwd_t(const void* gu, long ldgu, void* h, long ldh, long M, int F, int act, hipStream_t s) {
  constexpr int W = GluVec<T>::W;
  const bool vec = F % W == 0 && ldgu % W == 0 && ldh % W == 0 && al16(gu) && al16(h);
  if (vec)
    hipLaunchKernelGGL((fm_glu_act_fwd_kernel<T, W>), dim3(fm_grid(M * (F / W))), dim3(256), 0, s, (const T*)gu, ldgu, (T*)h,
                       ldh, M, F, act);
  else
    hipLaunchKernelGGL((fm_glu_act_fwd_kernel<T, 1>), dim3(fm_grid(M * F)), dim3(256), 0, s, (const T*)gu, ldgu, (T*)h, ldh,
                       M, F, act);
}

template <typename T>
void glu_act_bwd_t(const void* dh, long lddh, const void* gu, long ldgu, void* dgu, long lddgu, long M, int F, int act,
                   hipStream_t s) {
  constexpr int W = GluVec<T>::W;
  const bool vec = F % W == 0 && lddh % W == 0 && ldgu % W == 0 && lddgu % W == 0 && al16(dh) && al16(gu) && al16(dgu);
  if (vec)
    hipLaunchKernelGGL((fm_glu_act_bwd_kernel<T, W>), dim3(fm_grid(M * (F / W))), dim3(256), 0, s, (const T*)dh, lddh,
                       (const T*)gu, ldgu, (T*)dgu, lddgu, M, F, act);
  else
    hipLaunchKernelGGL((fm_glu_act_bwd_kernel<T, 1>), dim3(fm_grid(M * F)), dim3(256), 0, s, (const T*)dh, lddh,
                       (const T*)gu, ldgu, (T*)dgu, lddgu, M, F, act);
}

}  // namespace

// What the fused forward takes: 16-B aligned bases, 16-B chunks along H, 8-B quads along F.
extern "C" int fm_glu_gemm_eligible(const void* x, long ldx, const void* w, const void* gu, const void* h, long ldh, long M,
                                    int F, int H) {
  return M >= 1 && M <= 0x7fffffffL - GBM && F >= 4 && F % 4 == 0 && H >= 8 && H % 8 == 0 && ldx >= H && ldx % 8 == 0 &&
         ldh >= F && ldh % 4 == 0 && al16(x) && al16(w) && al16(gu) && al16(h);
}

// 0: launched; 1: refused (fm_glu_gemm_eligible, or an activation that is neither 0 = SiLU nor 1 = GELU)
extern "C" int fm_glu_gemm_fwd(const void* x, long ldx, const void* w, void* gu, void* h, long ldh, long M, int F, int H,
                               int act, hipStream_t stream) {
  if (M == 0) return 0;
  if ((act != GLU_SILU && act != GLU_GELU) || !fm_glu_gemm_eligible(x, ldx, w, gu, h, ldh, M, F, H)) return 1;
  GluP p;
  p.x = (const unsigned short*)x; p.ldx = ldx;
  p.w = (const unsigned short*)w;
  p.gu = (unsigned short*)gu;
  p.h = (unsigned short*)h; p.ldh = ldh;
  p.M = (int)M; p.F = F; p.H = H; p.act = act;
  p.tiles_m = (int)((M + GBM - 1) / GBM);
  p.tiles_n = (F + GBN - 1) / GBN;
  const long tiles = (long)p.tiles_m * p.tiles_n;
  if (tiles > 0x7fffffffL) return 1;
  const bool dma = fm_gemm_dma_enabled() && M % GBM == 0 && F % GBN == 0 && H % BK == 0;
  if (dma) hipLaunchKernelGGL(fm_glu_gemm_kernel<true>, dim3((unsigned)tiles), dim3(GNT), 2 * STAGE_BYTES, stream, p);
  else hipLaunchKernelGGL(fm_glu_gemm_kernel<false>, dim3((unsigned)tiles), dim3(GNT), 2 * STAGE_BYTES, stream, p);
  return 0;
}

// 0: launched; 1: refused (a row stride shorter than the row, or an unknown activation)
extern "C" int fm_glu_act_fwd(const void* gu, long ldgu, void* h, long ldh, long M, int F, int act, int bf16,
                              hipStream_t stream) {
  if (M <= 0 || F <= 0) return M < 0 || F < 0;
  if ((act != GLU_SILU && act != GLU_GELU) || ldgu < 2L * F || ldh < F) return 1;
  if (bf16) glu_act_fwd_t<unsigned short>(gu, ldgu, h, ldh, M, F, act, stream);
  else glu_act_fwd_t<float>(gu, ldgu, h, ldh, M, F, act, stream);
  return 0;
}

extern "C" int fm_glu_act_bwd(const void* dh, long lddh, const void* gu, long ldgu, void* dgu, long lddgu, long M, int F,
                              int act, int bf16, hipStream_t stream) {
  if (M <= 0 || F <= 0) return M < 0 || F < 0;
  if ((act != GLU_SILU && act != GLU_GELU) || lddh < F || ldgu < 2L * F || lddgu < 2L * F) return 1;
  if (bf16) glu_act_bwd_t<unsigned short>(dh, lddh, gu, ldgu, dgu, lddgu, M, F, act, stream);
  else glu_act_bwd_t<float>(dh, lddh, gu, ldgu, dgu, lddgu, M, F, act, stream);
  return 0;
}
