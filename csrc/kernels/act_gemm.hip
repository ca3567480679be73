// Dense layer with a non-monotonic activation (exact GELU, tanh-GELU, SiLU) for gfx950 (MI355X / CDNA4).
//
//   z[M, F] = x[M, H] W[F, H]^T + b      rounded to bf16 ONCE and kept ("pre"): the backward needs it,
//   y[M, F] = act(z)                     because act' is no function of y
//
// fm_act_gemm_fwd is the fused forward on bf16 operands: ONE MFMA GEMM that writes z and y, with no pass over
// memory in between.  A block of four waves (2 x 2) owns a 128 x BN tile, BN = 128 or 64 (template NR = 4 or 2
// 16-column subtiles per wave; the launcher's `tile` argument picks, tools/bench_act_linear.py measures both).
// Per 64-deep k step it stages x [128][64] and W [BN][64] as K-contiguous XOR-swizzled images (gemm_common.h),
// double-buffered: 64 KiB of LDS at BN = 128, 48 KiB at 64.  A wave holds 64 rows x 16 NR columns in ONE
// accumulator set (4 x NR tiles of v_mfma_f32_16x16x32_bf16, 64 or 32 fp32 accumulators).  The MFMA operands
// are swapped (weight fragment as "A"), so a lane owns 4 consecutive columns of a row: the epilogue loads its
// 4 bias values per column group once (16 B, hoisted out of the row loop), adds them, rounds z to bf16 and
// stores 8 B into pre, evaluates the activation in fp32 FROM THE ROUNDED z and stores 8 B into y.  The
// activation is a wave-uniform runtime code (act_math.h).  Full tiles stage by LDS-DMA (each lane loads the
// 16-B chunk the swizzle puts at its slot), every other legal shape through registers with zero-filled edge
// chunks and masked stores (template switch DMA).  Tile order is XCD-aware.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no instantiation uses scratch or spills):
//   <DMA, NR = 4>  116 VGPR    <DMA, NR = 2>   74 VGPR    (0 AGPR, 65536 / 49152 B dynamic LDS)
//   <reg, NR = 4>  158 VGPR    <reg, NR = 2>  106 VGPR
//   fm_act_bwd_kernel 33 to 41 VGPR, 1 to 8 KiB static LDS; the fold 18 VGPR
//
// fm_act_bwd is the element-wise half of the backward, bf16 and fp32:  dz = dy * act'(z) from the stored z,
// written to dpre, and the bias gradient db += column sums of the fp32 dz WITHOUT atomics: a block owns
// ACT_BWD_ROWS rows of a column tile, its 8 row lanes keep fp32 column partials in registers, fold them through
// LDS in a fixed order and write ONE partial row per block into a workspace; fm_act_bwd_fold_kernel then sums
// the partial rows of a column in block order into db.  The result does not depend on scheduling.  16-byte
// accesses; an element path (W = 1) serves widths that are no multiple of the vector and misaligned operands.
// dX and dW are ordinary GEMMs over dpre.
#include "act_math.h"
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// fused forward
constexpr int ANT = 256;                       // 4 waves, 2 x 2
constexpr int ABM = 128;                       // rows of a block tile
constexpr int AX_BYTES = ABM * BK * 2;         // 16 KiB

struct ActP {
  const unsigned short* x; long ldx;
  const unsigned short* w;                     // [F][H], contiguous
  const float* bias;                           // [F] or null
  unsigned short* pre;                         // [M][F], contiguous
  unsigned short* y; long ldy;
  int M, F, H, code;
  int tiles_m, tiles_n;
};

// global -> registers of one K-contiguous operand tile [R][64]: 16-B chunks, zero-filled past the edges
template <int R>
struct ActStage {
  static constexpr int PER_T = R * BK / 8 / ANT;
  u32x4_t v[PER_T];

  FM_DEVICE void load(const unsigned short* __restrict__ p, long ld, int row0, int rows, int k0, int K, int tid) {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + ANT * i;
      const int gr = row0 + (ci >> 3), gk = k0 + 8 * (ci & 7);
      // K % 8 == 0 (launcher): a chunk is wholly inside or wholly outside the row
      v[i] = (gr < rows && gk < K) ? *reinterpret_cast<const u32x4_t*>(p + (long)gr * ld + gk) : u32x4_t{0u, 0u, 0u, 0u};
    }
  }
  FM_DEVICE void store(char* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int ci = tid + ANT * i;
      *reinterpret_cast<u32x4_t*>(lds + lds_off<true, R>(ci >> 3, ci & 7)) = v[i];
    }
  }
};

// global -> LDS by LDS-DMA, full tiles only: one wave-instruction fills 1 KiB of the image, lane L's 16 B land
// at piece + 16 L, so the lane loads the chunk the swizzle puts there (the inverse of lds_off)
template <int R>
FM_DEVICE void act_dma(const unsigned short* __restrict__ p, long ld, int row0, int k0, char* lds, int wave, int lane) {
  constexpr int PER_W = R * BK * 2 / 1024 / (ANT / 64);
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

template <bool DMA, int NR>
__global__ void __launch_bounds__(ANT, 2) fm_act_gemm_kernel(ActP p) {
  constexpr int MR = 4;                        // 16 x 16 subtiles of a wave: 64 rows x 16 NR columns
  constexpr int BN = 32 * NR;
  constexpr int STAGE_BYTES = AX_BYTES + BN * BK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
#define LDS_X(b) (smem + (b) * STAGE_BYTES)
#define LDS_W(b) (smem + (b) * STAGE_BYTES + AX_BYTES)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware order; column tiles fastest, so the blocks of one XCD share an x row tile
  const int bid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
  const int m0 = (bid / p.tiles_n) * ABM, n0 = (bid % p.tiles_n) * BN;
  const int ktiles = (p.H + BK - 1) / BK;

  f32x4_t acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  ActStage<ABM> sx;
  ActStage<BN> sw;
  auto stage_dma = [&](int kt, int b) {
    act_dma<ABM>(p.x, p.ldx, m0, kt * BK, LDS_X(b), wave, lane);
    act_dma<BN>(p.w, p.H, n0, kt * BK, LDS_W(b), wave, lane);
  };
  auto stage_load = [&](int kt) {
    sx.load(p.x, p.ldx, m0, p.M, kt * BK, p.H, tid);
    sw.load(p.w, p.H, n0, p.F, kt * BK, p.H, tid);
  };
  auto stage_store = [&](int b) {
    sx.store(LDS_X(b), tid);
    sw.store(LDS_W(b), tid);
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
    const char* lw = LDS_W(cur);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8_t xf[MR], wf[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) xf[i] = frag<true, ABM>(lx, wm * 64 + 16 * i, kk, lane);
#pragma unroll
      for (int j = 0; j < NR; ++j) wf[j] = frag<true, BN>(lw, wn * 16 * NR + 16 * j, kk, lane);
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
          // operands swapped (weight fragment as the MFMA "A"): a lane owns 4 consecutive columns
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8v_t*>(&wf[j]),
                                                              *reinterpret_cast<bf16x8v_t*>(&xf[i]), acc[i][j], 0, 0, 0);
    }
    if constexpr (DMA) {
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's pieces of step kt + 1 landed
    } else if (more) {
      stage_store(cur ^ 1);
    }
    __syncthreads();
  }
#undef LDS_X
#undef LDS_W

  // epilogue: lane (q, g4) holds z of row 16 i + q, columns 16 j + 4 g4 .. + 3 of the wave tile.
  // F % 4 == 0 (launcher): a quad is wholly inside or wholly outside
  const int q = lane & 15, g4 = lane >> 4;
  f32x4_t bq[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int n = n0 + wn * 16 * NR + 16 * j + 4 * g4;
    bq[j] = (p.bias != nullptr && (DMA || n < p.F)) ? *reinterpret_cast<const f32x4_t*>(p.bias + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    const int m = m0 + wm * 64 + 16 * i + q;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int n = n0 + wn * 16 * NR + 16 * j + 4 * g4;
      if (!DMA && (m >= p.M || n >= p.F)) continue;
      bf16x4_t zq, yq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned short zb = f2bf(acc[i][j][r] + bq[j][r]);
        zq[r] = (short)zb;
        yq[r] = (short)f2bf(actz_fwd(p.code, bf2f(zb)));
      }
      *reinterpret_cast<bf16x4_t*>(p.pre + (long)m * p.F + n) = zq;
      *reinterpret_cast<bf16x4_t*>(p.y + (long)m * p.ldy + n) = yq;
    }
  }
}

template <bool DMA, int NR>
void act_gemm_launch(const ActP& p, long tiles, hipStream_t stream) {
  constexpr int lds = 2 * (AX_BYTES + 32 * NR * BK * 2);
  hipLaunchKernelGGL((fm_act_gemm_kernel<DMA, NR>), dim3((unsigned)tiles), dim3(ANT), lds, stream, p);
}

// ------------------------------------------------------------------------------------------------
// backward: dz = dy * act'(z), db partial rows
constexpr int ACT_BWD_ROWS = 64;               // rows of a block: 8 row lanes x 8 steps
constexpr int BWD_CG = 32;                     // column groups of W elements per block

template <typename T> struct ActVec;
template <> struct ActVec<unsigned short> { static constexpr int W = 8; };
template <> struct ActVec<float> { static constexpr int W = 4; };

template <int W, typename T>
FM_DEVICE void act_ld(const T* p, float (&v)[W]) {
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
FM_DEVICE void act_st(T* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    st8<T>(p, v);
  } else if constexpr (W == 4) {
    *reinterpret_cast<f32x4_t*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
  } else {
    st<T>(p, v[0]);
  }
}

// block b = (row block rb, column tile ct), column tiles fastest.  part (null: no bias gradient) takes row rb.
template <typename T, int W>
__global__ void __launch_bounds__(256) fm_act_bwd_kernel(const T* __restrict__ dy, long lddy, const T* __restrict__ pre, long ldp,
                                                        T* __restrict__ dpre, long lddp, float* __restrict__ part, long M, int F,
                                                        int ctiles, int code) {
  __shared__ float red[8][BWD_CG * W];
  const int tx = threadIdx.x & (BWD_CG - 1), ty = threadIdx.x / BWD_CG;
  const long rb = blockIdx.x / ctiles;
  const int ct = blockIdx.x % ctiles;
  const long c = ((long)ct * BWD_CG + tx) * W;       // F % W == 0: a group is wholly inside or wholly outside
  float acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = 0.f;
  if (c < F) {
#pragma unroll
    for (int it = 0; it < ACT_BWD_ROWS / 8; ++it) {
      const long r = rb * ACT_BWD_ROWS + ty + 8 * it;
      if (r < M) {
        float d[W], z[W];
        act_ld<W, T>(dy + r * lddy + c, d);
        act_ld<W, T>(pre + r * ldp + c, z);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          d[j] *= actz_dfwd(code, z[j]);
          acc[j] += d[j];
        }
        act_st<W, T>(dpre + r * lddp + c, d);
      }
    }
  }
  if (part == nullptr) return;
#pragma unroll
  for (int j = 0; j < W; ++j) red[ty][tx * W + j] = acc[j];
  __syncthreads();
  for (int col = threadIdx.x; col < BWD_CG * W; col += 256) {
    const long gc = (long)ct * BWD_CG * W + col;
    if (gc < F) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += red[k][col];
      part[rb * F + gc] = s;
    }
  }
}

// db[c] += the partial rows of column c, in row-block order
__global__ void __launch_bounds__(256) fm_act_bwd_fold_kernel(const float* __restrict__ part, float* __restrict__ db, int F, int nrb) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c < F) db[c] += slab_sum1(part + c, F, nrb);
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <typename T>
int act_bwd_t(const void* dy, long lddy, const void* pre, long ldp, void* dpre, long lddp, float* db, float* ws, long ws_bytes,
              long M, int F, int code, hipStream_t s) {
  constexpr int W = ActVec<T>::W;
  const bool vec = F % W == 0 && lddy % W == 0 && ldp % W == 0 && lddp % W == 0 && al16(dy) && al16(pre) && al16(dpre);
  const int cols = BWD_CG * (vec ? W : 1);
  const long ctiles = ((long)F + cols - 1) / cols, nrb = (M + ACT_BWD_ROWS - 1) / ACT_BWD_ROWS;
  if (ctiles * nrb > 0x7fffffffL || nrb > 0x7fffffffL) return 1;
  if (db != nullptr && (ws == nullptr || ws_bytes < nrb * F * 4)) return 2;
  float* part = db != nullptr ? ws : nullptr;
  if (vec)
    hipLaunchKernelGGL((fm_act_bwd_kernel<T, W>), dim3((unsigned)(ctiles * nrb)), dim3(256), 0, s, (const T*)dy, lddy, (const T*)pre,
                       ldp, (T*)dpre, lddp, part, M, F, (int)ctiles, code);
  else
    hipLaunchKernelGGL((fm_act_bwd_kernel<T, 1>), dim3((unsigned)(ctiles * nrb)), dim3(256), 0, s, (const T*)dy, lddy, (const T*)pre,
                       ldp, (T*)dpre, lddp, part, M, F, (int)ctiles, code);
  if (db != nullptr)
    hipLaunchKernelGGL(fm_act_bwd_fold_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, part, db, F, (int)nrb);
  return 0;
}

}  // namespace

// What the fused forward takes: 16-B aligned bases, 16-B chunks along H, 8-B quads along F.
extern "C" int fm_act_gemm_eligible(const void* x, long ldx, const void* w, const float* bias, const void* pre, const void* y,
                                    long ldy, long M, int F, int H) {
  return M >= 1 && M <= 0x7fffffffL - ABM && F >= 4 && F % 4 == 0 && F <= 0x7fffffff - 128 && H >= 8 && H % 8 == 0 &&
         H <= 0x7fffffff - BK && ldx >= H && ldx % 8 == 0 && ldy >= F && ldy % 4 == 0 && al16(x) && al16(w) && al16(bias) &&
         al16(pre) && al16(y);
}

// tile: columns of a block tile, 128 or 64; 0 = the default.  0: launched; 1: refused (fm_act_gemm_eligible, an
// activation code outside 5..7, or another tile)
extern "C" int fm_act_gemm_fwd(const void* x, long ldx, const void* w, const float* bias, void* pre, void* y, long ldy, long M,
                               int F, int H, int code, int tile, hipStream_t stream) {
  if (M == 0) return 0;
  if (tile == 0) tile = 128;
  if (!actz_known(code) || (tile != 64 && tile != 128) || !fm_act_gemm_eligible(x, ldx, w, bias, pre, y, ldy, M, F, H)) return 1;
  ActP p;
  p.x = (const unsigned short*)x; p.ldx = ldx;
  p.w = (const unsigned short*)w;
  p.bias = bias;
  p.pre = (unsigned short*)pre;
  p.y = (unsigned short*)y; p.ldy = ldy;
  p.M = (int)M; p.F = F; p.H = H; p.code = code;
  p.tiles_m = (int)((M + ABM - 1) / ABM);
  p.tiles_n = (F + tile - 1) / tile;
  const long tiles = (long)p.tiles_m * p.tiles_n;
  if (tiles > 0x7fffffffL) return 1;
  const bool dma = fm_gemm_dma_enabled() && M % ABM == 0 && F % tile == 0 && H % BK == 0;
  if (tile == 128) {
    if (dma) act_gemm_launch<true, 4>(p, tiles, stream);
    else act_gemm_launch<false, 4>(p, tiles, stream);
  } else {
    if (dma) act_gemm_launch<true, 2>(p, tiles, stream);
    else act_gemm_launch<false, 2>(p, tiles, stream);
  }
  return 0;
}

// rows of dz that one block of fm_act_bwd sums into one partial row of the bias gradient
extern "C" int fm_act_bwd_rows() { return ACT_BWD_ROWS; }

// dpre = dy * act'(pre); db (fp32 [F], null: not formed) += column sums of the fp32 products, through ws of at
// least ceil(M / fm_act_bwd_rows()) * F floats.  0: launched; 1: refused (row stride shorter than the row,
// activation code outside 5..7, too many blocks); 2: workspace too small
extern "C" int fm_act_bwd(const void* dy, long lddy, const void* pre, long ldp, void* dpre, long lddp, float* db, float* ws,
                          long ws_bytes, long M, int F, int code, int bf16, hipStream_t stream) {
  if (M <= 0 || F <= 0) return M < 0 || F < 0;
  if (!actz_known(code) || lddy < F || ldp < F || lddp < F) return 1;
  return bf16 ? act_bwd_t<unsigned short>(dy, lddy, pre, ldp, dpre, lddp, db, ws, ws_bytes, M, F, code, stream)
              : act_bwd_t<float>(dy, lddy, pre, ldp, dpre, lddp, db, ws, ws_bytes, M, F, code, stream);
}
