// The one output rule of flexmi's MFMA GEMMs (gemm.hip bf16, gemm_f32.hip / gemm_x3.hip fp32) and
// everything that applies it: the parameter blocks, the tile epilogue (split-K slab store, wave-shuffle
// column sums, LDS-staged fused SGD) and the split-K reduce kernels with their launch helper.
//
// What a GEMM does with a finished fp32 sum s of output element (m, n):
//   v = act_fwd(act, s * alpha + bias[n])
//   if ay:      v = act_bwd(bact, ay[m][n], v)          fused activation backward of the layer below
//   if colsum:  colsum[n] += v                          its bias gradient (the unrounded value)
//   then        fused SGD on W at (m, n) with gradient v (update_rule.h)
//      or       C[m][n] = round_to_C_type(v + (beta ? C[m][n] : 0))
// gemm_out below is the only place this is written.  Two parts of it are compiled in only where a GEMM
// can reach them.  Fused-SGD GEMMs are weight gradients (fm_gemm_dw_sgd / fm_gemm_f32_dw_sgd pass no
// bias, activation, ay or colsum): their instantiations take v = s * alpha and nothing else, in the tile
// epilogue as in sgd_epilogue_lds and the reduces.  The ay / colsum lines exist in the tile epilogue and in
// fm_gemm_reduce_bwd only: the host sends every split GEMM that carries them to that reduce.
// The two families differ in element types only: ay is bf16 or fp32, C is fp32 or (bf16 family,
// p.c_fp32 == 0) bf16.
#pragma once
#include "gemm_common.h"
#include "update_rule.h"

#include <algorithm>

// The fields both parameter blocks share.
struct GemmEp {
  long ldc; long sC;
  const float* bias;
  float* ws;          // split-K slabs [batch][split][M][N]
  // fused backward epilogue of the producing layer below: v = act'(ay) * v ; colsum[n] += sum_m v
  long lday;
  float* colsum;
  float* rowsum_a;   // += sum_k A(m,k)  (MN-contiguous A only; used for bias grads in dW GEMMs)
  int bact;
  int M, N, K, act, beta, ksplit, batch;
  float alpha;
  int tiles_m, tiles_n;
  int n_fast;   // tile order: column tiles fastest (A row-block reused by consecutive tiles on one XCD)
  // fused SGD (dW GEMMs whose gradient has no other consumer): instead of storing the gradient,
  // the epilogue updates the fp32 master W (same [M][ldc] layout as C), its momentum and bf16 mirror
  // by the rule of update_rule.h -- the gradient never round-trips through HBM
  float* uw;             // nullptr = plain GEMM
  unsigned short* uwc;   // bf16 compute mirror (nullptr: none)
  float* uv;             // momentum buffer (used when umom > 0)
  const float* ulr;      // device-side learning rate
  float uwd, umom;
  int unest;
  int ulds;              // unsplit tiles stage the update through LDS (sgd_epilogue_lds)
  int dma;               // operands staged by LDS-DMA (full tiles, no row sums)
};

// bf16 operands (gemm.hip)
struct GemmP : GemmEp {
  const unsigned short* A; long lda; long sA;
  const unsigned short* B; long ldb; long sB;
  void* C;
  const unsigned short* ay;
  int c_fp32;   // C holds fp32, else bf16
  static constexpr bool kDeepReduce = false;   // every vector split-K reduce is the plain one
};

// fp32 operands and output (gemm_f32.hip, gemm_x3.hip)
struct GemmF : GemmEp {
  const float* A; long lda; long sA;
  const float* B; long ldb; long sB;
  float* C;
  const float* ay;
  // fp16 two-plane split (gemm_x3.hip F16 form): max |x| bit patterns of every A row (M index) and
  // every B column (N index) over K, from fm_f32_amax (the per-row / per-column power-of-two scales)
  const unsigned* amax_a;
  const unsigned* amax_b;
  int amax_na, amax_nb;   // partials per index (strides M / N): the scale takes their max
  static constexpr bool kDeepReduce = true;    // ks >= 16 vector reduces run fm_gemm_reduce_deep
};

// The optimizer state of a fused-SGD dW GEMM (fm_gemm_dw_sgd / fm_gemm_f32_dw_sgd).
struct SgdUpd {
  float* w; unsigned short* wc; float* v; const float* lr; float wd, mom; int nest;
};

// the fused epilogue's 16-B accesses need ldc % 4 == 0 and aligned W / V (16 B) and mirror (8 B)
static inline bool sgd_upd_ok(const SgdUpd& u, int K, long ldc) {
  return K > 0 && ldc % 4 == 0 && !(((uintptr_t)u.w | (uintptr_t)(u.v ? u.v : u.w)) & 15) &&
         !(((uintptr_t)(u.wc ? (void*)u.wc : (void*)u.w)) & 7);
}

static inline void gemm_set_update(GemmEp& p, const SgdUpd* upd) {
  const SgdUpd u = upd ? *upd : SgdUpd{nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0};
  p.uw = u.w; p.uwc = u.wc; p.uv = u.v; p.ulr = u.lr; p.uwd = u.wd; p.umom = u.mom; p.unest = u.nest;
  p.ulds = upd != nullptr;   // the update staged through LDS (whole-row W accesses, sgd_epilogue_lds)
}

// the split-bf16 kernel (gemm_x3.hip) on a parameter block prepared by gemm_f32.hip
extern "C" int fm_gemm_x3v2_launch(const GemmF* p, int bm, int bn, int a_kcontig, int b_kcontig, int sgd, hipStream_t s);

// Up to GEMM_GROUP_MAX fp32 problems run by one grid (gemm_x3.hip fm_gemm_x3v2_grouped_kernel, then
// fm_gemm_reduce_grouped below): problem g owns the flat block ids [first[g], first[g + 1]) of the
// launch the struct is passed to (the GEMM's blocks or the reduce's) and keeps its split-K slabs
// [ksplit][M][N] at its own 16-B aligned p[g].ws.  vec[g]: the reduce takes problem g four outputs at
// a time (the v4 rule of launch_splitk_reduce).
constexpr int GEMM_GROUP_MAX = 4;
struct GemmFGroup {
  GemmF p[GEMM_GROUP_MAX];
  int first[GEMM_GROUP_MAX + 1];
  int vec[GEMM_GROUP_MAX];
  int n;
};
extern "C" int fm_gemm_x3v2_launch_grouped(const GemmFGroup* g, int a_kcontig, int b_kcontig, hipStream_t s);

namespace {

// The SGD step on W at offset o with gradient g, by update_rule.h's rule
FM_DEVICE void sgd_apply1(const GemmEp& p, long o, float g) {
  update_lanes(SgdRule{p.uwd, p.umom, p.unest}, UpdBufs<SgdRule>{p.uw, {p.uv}, p.uwc}, p.ulr[0], o, g);
}

// four consecutive elements at a 16-B aligned offset o
FM_DEVICE void sgd_apply4(const GemmEp& p, long o, f32x4_t g) {
  update_lanes(SgdRule{p.uwd, p.umom, p.unest}, UpdBufs<SgdRule>{p.uw, {p.uv}, p.uwc}, p.ulr[0], o, g);
}

// tile coordinates of remapped block id: consecutive ids share an XCD (xcd_remap), so the
// operand traversed slowest stays resident in that XCD's 4 MB L2 while the other streams
struct TileMN {
  int m, n;
};
FM_DEVICE TileMN tile_coords(const GemmEp& p, int bid) {
  TileMN t;
  if (p.n_fast) { t.n = bid % p.tiles_n; t.m = bid / p.tiles_n; }
  else { t.m = bid % p.tiles_m; t.n = bid / p.tiles_m; }
  return t;
}

// ---- the output rule --------------------------------------------------------------------------
// four consecutive elements as fp32 from fp32 / bf16 storage (one 16-B / 8-B access)
FM_DEVICE f32x4_t ld4(const float* s) { return *reinterpret_cast<const f32x4_t*>(s); }
FM_DEVICE f32x4_t ld4(const unsigned short* s) {
  const bf16x4_t t = *reinterpret_cast<const bf16x4_t*>(s);
  return f32x4_t{bf2f((unsigned short)t[0]), bf2f((unsigned short)t[1]), bf2f((unsigned short)t[2]),
                 bf2f((unsigned short)t[3])};
}
FM_DEVICE void st4(float* d, f32x4_t v) { *reinterpret_cast<f32x4_t*>(d) = v; }
FM_DEVICE void st4(unsigned short* d, f32x4_t v) {
  *reinterpret_cast<bf16x4_t*>(d) = bf16x4_t{(short)f2bf(v[0]), (short)f2bf(v[1]), (short)f2bf(v[2]), (short)f2bf(v[3])};
}

// How a quad reaches ay and C: Q_ANY decides per quad (full, leading dimension, address), as the tile
// epilogue must; Q_VEC / Q_SCALAR: the caller decided once for all its quads (the split-K reduces: the
// host or the thread checked that every quad is full and aligned, or falls back to scalar accesses)
enum { Q_ANY = 0, Q_VEC = 1, Q_SCALAR = 2 };

// C[0..W) = round(v + (beta ? C : 0)) for the columns that exist (full, or n0 + e < N)
template <int W, int FORM, class T>
FM_DEVICE void c_store_at(T* dst, const float (&v)[W], const GemmEp& p, int n0, bool full) {
  if constexpr (W == 4 && FORM != Q_SCALAR) {
    if (FORM == Q_VEC || (full && ((p.ldc & 3) == 0) && ((((uintptr_t)dst) & (4 * sizeof(T) - 1)) == 0))) {
      f32x4_t o = {v[0], v[1], v[2], v[3]};
      if (p.beta) o += ld4(dst);
      st4(dst, o);
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e)
    if (full || n0 + e < p.N) st<T>(dst + e, v[e] + (p.beta ? ld<T>(dst + e) : 0.f));
}
template <int W, int FORM>
FM_DEVICE void c_store(const GemmF& p, long ci, const float (&v)[W], int n0, bool full) {
  c_store_at<W, FORM>(p.C + ci, v, p, n0, full);
}
template <int W, int FORM>
FM_DEVICE void c_store(const GemmP& p, long ci, const float (&v)[W], int n0, bool full) {
  if (p.c_fp32) c_store_at<W, FORM>(reinterpret_cast<float*>(p.C) + ci, v, p, n0, full);
  else c_store_at<W, FORM>(reinterpret_cast<unsigned short*>(p.C) + ci, v, p, n0, full);
}


// The rule for W (4, or 1 in the scalar reduce) consecutive columns n0.. of row m < M of batch zb:
// v holds the finished sums on entry and the values the columns contributed on exit; full = all W
// columns exist (else column n0 + e exists iff n0 + e < N; Q_VEC implies full); BWD: the fused backward
// lines, cs += the column-sum contributions (untouched without BWD).
template <int W, bool SGD, bool BWD, int FORM = Q_ANY, class P>
FM_DEVICE void gemm_out(const P& p, int zb, int m, int n0, bool full, float (&v)[W], float (&cs)[W]) {
  static_assert(W == 1 || W == 4, "one element or a quad");
  auto ok = [&](int e) { return FORM == Q_VEC || full || n0 + e < p.N; };
  if constexpr (SGD) {
    // v = s * alpha only (see the head of this file); the host guarantees ldc % 4 == 0 and 16-B aligned W / V / C
    const long o = (long)m * p.ldc + n0;
    if constexpr (W == 4 && FORM != Q_SCALAR) {
      if (FORM == Q_VEC || full) {
        sgd_apply4(p, o, f32x4_t{v[0], v[1], v[2], v[3]} * p.alpha);
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e)
      if (ok(e)) sgd_apply1(p, o + e, v[e] * p.alpha);
    return;
  }
  float b[W] = {};
  if (p.bias) {
#pragma unroll
    for (int e = 0; e < W; ++e) b[e] = ok(e) ? p.bias[n0 + e] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < W; ++e) v[e] = act_fwd(p.act, v[e] * p.alpha + b[e]);
  if constexpr (BWD) {
    if (p.ay) {  // fused activation backward of the layer below (dX -> dpre)
      const auto* yp = p.ay + (long)m * p.lday + n0;
      float yv[W];
      bool vec = false;
      if constexpr (W == 4 && FORM != Q_SCALAR) vec = FORM == Q_VEC || (full && ((p.lday & 3) == 0));
      if (vec) {
        const f32x4_t t = ld4(yp);
#pragma unroll
        for (int e = 0; e < W; ++e) yv[e] = t[e];
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) yv[e] = ok(e) ? tof(yp[e]) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < W; ++e) v[e] = act_bwd(p.bact, yv[e], v[e]);
    }
    if (p.colsum) {
#pragma unroll
      for (int e = 0; e < W; ++e) cs[e] += ok(e) ? v[e] : 0.f;
    }
  }
  c_store<W, FORM>(p, (long)zb * p.sC + (long)m * p.ldc + n0, v, n0, full);
}

// ---- tile epilogue ------------------------------------------------------------------------------
// lane (q = lane&15, g = lane>>4) holds acc[i][j][r] = C[m(i, q)][n(j, 4g + r)] with
//   m = IL_A ? mbase + MR*q + i : mbase + 16i + q          (IL = the fp32 kernel's MN-contiguous operand)
//   n = IL_B ? nbase + NR*qn + j : nbase + 16j + qn        (qn = 4g + r)
// processed as NR quads of 4 consecutive columns per row.  The bf16 kernel and the split kernel hold the
// plain layout (IL_A = IL_B = false): lane owns C[m][n..n+3], m = lane&15, n = 4*(lane>>4) of each 16x16 tile.
template <int MR, bool IL_A>
FM_DEVICE int acc_row(int i, int mbase, int q) {
  return IL_A ? mbase + MR * q + i : mbase + 16 * i + q;
}
template <int MR, int NR, bool IL_B>
FM_DEVICE void quad_of(const f32x4_t (&acc)[MR][NR], int i, int u, int nbase, int g, int& n0, float (&v)[4]) {
  if constexpr (IL_B) {
    n0 = nbase + 4 * NR * g + 4 * u;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[i][(4 * u + e) % NR][(4 * u + e) / NR];
  } else {
    n0 = nbase + 16 * u + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[i][u][e];
  }
}

// SGD: the fused-SGD instantiation (dW GEMMs of fm_gemm_dw_sgd / fm_gemm_f32_dw_sgd); plain GEMMs
// compile without it
template <int MR, int NR, bool IL_A, bool IL_B, bool SGD, class P>
FM_DEVICE void gemm_epilogue(const P& p, const f32x4_t (&acc)[MR][NR], int zb, int split, int mbase, int nbase, int lane) {
  const int q = lane & 15, g = lane >> 4;
  if (p.ksplit > 1) {   // split-K partial tile -> fp32 slab [batch][split][M][N] (reduce launch)
    float* ws = p.ws + ((long)zb * p.ksplit + split) * (long)p.M * p.N;
    const bool v4 = (p.N & 3) == 0;
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int m = acc_row<MR, IL_A>(i, mbase, q);
      if (m >= p.M) continue;
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        int n0;
        float v[4];
        quad_of<MR, NR, IL_B>(acc, i, u, nbase, g, n0, v);
        float* dst = ws + (long)m * p.N + n0;
        if (v4 && n0 + 3 < p.N) {
          *reinterpret_cast<f32x4_t*>(dst) = f32x4_t{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n0 + e < p.N) dst[e] = v[e];
        }
      }
    }
    return;
  }
  float csum[NR][4];
#pragma unroll
  for (int u = 0; u < NR; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[u][e] = 0.f;
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    const int m = acc_row<MR, IL_A>(i, mbase, q);
    if (m >= p.M) continue;
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      int n0;
      float v[4];
      quad_of<MR, NR, IL_B>(acc, i, u, nbase, g, n0, v);
      gemm_out<4, SGD, true>(p, zb, m, n0, n0 + 3 < p.N, v, csum[u]);
    }
  }
  if (p.colsum) {   // the 16 lanes of a group share every column: reduce over q, one atomic per column
#pragma unroll
    for (int u = 0; u < NR; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = csum[u][e];
        x += __shfl_xor(x, 1, 64);
        x += __shfl_xor(x, 2, 64);
        x += __shfl_xor(x, 4, 64);
        x += __shfl_xor(x, 8, 64);
        const int n = (IL_B ? nbase + 4 * NR * g + 4 * u : nbase + 16 * u + 4 * g) + e;
        if (q == 0 && n < p.N) atomicAdd(p.colsum + n, x);
      }
  }
}

// Fused-SGD epilogue of an unsplit dW tile, staged through LDS: the accumulator layout gives each
// lane 4 columns of one row, i.e. 64-B row pieces per 16x16 tile -- a scattered pattern that held the
// W read-modify-write (fp32 master + bf16 mirror, ~10 B per element) at ~2.8 TB/s.  The waves first
// park the BM x BN fp32 tile (the accumulator quads of quad_of, incl. the interleaved layouts) in the
// (free) operand LDS, 16-B chunks XOR-swizzled by row so both the accumulator writes and the row reads
// stay conflict-light, then every wave updates whole rows: BN*4 contiguous bytes of W per row (512 B
// for BN = 128).  LDSB = the kernel's K-loop LDS, which the tile fits (BM*BN*4 <= 2*(BM+BN)*BK*2 for
// bf16, 2*(BM+BN)*BKF*4 for fp32).
template <int BM, int BN, int NT, int MR, int NR, bool IL_A, bool IL_B, int LDSB>
FM_DEVICE void sgd_epilogue_lds(const GemmEp& p, const f32x4_t (&acc)[MR][NR], char* smem, int m0, int n0, int mbase,
                                int nbase, int lane, int tid) {
  constexpr int CPR = BN / 4;                       // 16-B chunks per tile row
  static_assert(BM * BN * 4 <= LDSB, "fp32 tile must fit the K-loop LDS");
  static_assert(CPR >= 8, "row XOR swizzle (r & 7) needs >= 8 chunks per row");
  f32x4_t* t = reinterpret_cast<f32x4_t*>(smem);
  const int q = lane & 15, g = lane >> 4;
  __syncthreads();                                  // every wave is done with the operand tiles
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    const int r = acc_row<MR, IL_A>(i, mbase, q) - m0;
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      int nn;
      float v[4];
      quad_of<MR, NR, IL_B>(acc, i, u, nbase, g, nn, v);
      const int c = (nn - n0) >> 2;
      t[r * CPR + (c ^ (r & 7))] = f32x4_t{v[0], v[1], v[2], v[3]} * p.alpha;
    }
  }
  __syncthreads();
  const bool n4 = (p.N & 3) == 0;
#pragma unroll 4
  for (int e = tid; e < BM * CPR; e += NT) {
    const int r = e / CPR, c = e % CPR;
    const int m = m0 + r, n = n0 + 4 * c;
    if (m >= p.M || n >= p.N) continue;
    const f32x4_t gv = t[r * CPR + (c ^ (r & 7))];
    const long o = (long)m * p.ldc + n;
    if (n4 && n + 3 < p.N) {
      sgd_apply4(p, o, gv);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (n + k < p.N) sgd_apply1(p, o + k, gv[k]);
    }
  }
}

// ---- split-K reduces: the slabs are fp32 whatever the operands were ----------------------------------
// plain reduce, W = 4 consecutive outputs per thread (16-B slab loads; the host checked N % 4 == 0 and a
// 16-B aligned fp32 C with ldc, sC % 4 == 0) or one.  GEMMs with a fused backward epilogue reduce in
// fm_gemm_reduce_bwd, so no column sums here.
template <class P, bool SGD, int W>
__global__ void fm_gemm_reduce(P p) {
  const long MN = (long)p.M * p.N;
  const long total = MN * p.batch / W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long e0 = i * W;
    const long zb = e0 / MN, e = e0 % MN;
    const int m = (int)(e / p.N), n = (int)(e % p.N);
    const float* src = p.ws + zb * p.ksplit * MN + e;
    float v[W], cs[W] = {};
    if constexpr (W == 4) {
      const f32x4_t s = slab_sum4(src, MN, p.ksplit);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = s[r];
    } else {
      v[0] = slab_sum1(src, MN, p.ksplit);
    }
    gemm_out<W, SGD, false, W == 4 ? Q_VEC : Q_SCALAR>(p, (int)zb, m, n, true, v, cs);
  }
}

// split-K reduce for DEEP splits (ks >= 16, v4 as above; the small-output dW GEMMs: 128 x 256 x 8192
// runs 64-way): the one-thread-per-4-outputs reduce above leaves a 32-block grid with 64 dependent
// slab reads per thread (21 us for 8 MB, profiles/prof_r5final_step_fp32.txt).  Here G = 8 threads
// share each 4-output group -- thread g sums slabs g, g + 8, ... in order -- and the G partial sums are
// added through LDS in g order (deterministic): 8x the blocks and the loads in flight.
constexpr int RD_G = 8;
template <class P, bool SGD>
__global__ void __launch_bounds__(256) fm_gemm_reduce_deep(P p) {
  __shared__ f32x4_t part[RD_G][256 / RD_G];
  constexpr int O = 256 / RD_G;
  const long MN = (long)p.M * p.N;
  const long total = MN * p.batch / 4;
  const int o = threadIdx.x % O, g = threadIdx.x / O;
  const long i = blockIdx.x * (long)O + o;
  const long e0 = (i < total ? i : total - 1) * 4;
  const long zb = e0 / MN, e = e0 % MN;
  const float* src = p.ws + zb * p.ksplit * MN + e;
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
  int k = g;
  for (; k + 3 * RD_G < p.ksplit; k += 4 * RD_G) {
    f32x4_t x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4_t*>(src + (long)(k + u * RD_G) * MN);
#pragma unroll
    for (int u = 0; u < 4; ++u) s += x[u];
  }
  for (; k < p.ksplit; k += RD_G) s += *reinterpret_cast<const f32x4_t*>(src + (long)k * MN);
  part[g][o] = s;
  __syncthreads();
  if (g != 0 || i >= total) return;
  s = part[0][o];
#pragma unroll
  for (int t = 1; t < RD_G; ++t) s += part[t][o];
  float v[4] = {s[0], s[1], s[2], s[3]}, cs[4] = {0.f, 0.f, 0.f, 0.f};
  gemm_out<4, SGD, false, Q_VEC>(p, (int)zb, (int)(e / p.N), (int)(e % p.N), true, v, cs);
}

// One reduce launch for the problems of a grouped GEMM (GemmFGroup, first[] = the reduce's own block
// ranges; an unsplit member has none: its tiles stored C themselves).  Every output goes through
// gemm_out like the single reduces, and a problem's slabs are added in the order the single reduce
// of its depth adds them -- slab order below 16 slabs (fm_gemm_reduce), RD_G interleaved partial
// sums added in g order from 16 up on quads (fm_gemm_reduce_deep) -- so the result is bit-identical
// to the ungrouped GEMM of the same form and depth.
template <class G>   // GemmFGroup (a template so that only the file that launches it compiles it)
__global__ void __launch_bounds__(256) fm_gemm_reduce_grouped(G s) {
  const int bid = blockIdx.x;
  int g = 0;
  for (int i = 1; i < s.n; ++i) g += bid >= s.first[i];      // first[] ascends: wave-uniform scan
  const auto& p = s.p[g];
  const int lb = bid - s.first[g], nb = s.first[g + 1] - s.first[g];
  const long MN = (long)p.M * p.N;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  if (s.vec[g]) {
    const bool deep = p.ksplit >= 16;
    for (long i = lb * 256L + threadIdx.x; i < MN / 4; i += nb * 256L) {
      const long e = i * 4;
      const float* src = p.ws + e;
      f32x4_t t;
      if (deep) {
        f32x4_t part[RD_G];
#pragma unroll
        for (int u = 0; u < RD_G; ++u) {
          part[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          for (int k = u; k < p.ksplit; k += RD_G) part[u] += *reinterpret_cast<const f32x4_t*>(src + (long)k * MN);
        }
        t = part[0];
#pragma unroll
        for (int u = 1; u < RD_G; ++u) t += part[u];
      } else {
        t = slab_sum4(src, MN, p.ksplit);
      }
      float v[4] = {t[0], t[1], t[2], t[3]};
      gemm_out<4, false, false, Q_VEC>(p, 0, (int)(e / p.N), (int)(e % p.N), true, v, cs);
    }
  } else {
    for (long e = lb * 256L + threadIdx.x; e < MN; e += nb * 256L) {
      float v[1] = {slab_sum1(p.ws + e, MN, p.ksplit)}, c1[1] = {0.f};
      gemm_out<1, false, false, Q_SCALAR>(p, 0, (int)(e / p.N), (int)(e % p.N), true, v, c1);
    }
  }
}

// The slab sums of the first nv of four adjacent columns, each column added in slab order as slab_sum1
// adds it, in one loop with four slabs in flight (four inlined slab_sum1 loops held their slab offsets in
// SGPRs four times over and spilled them)
FM_DEVICE void slab_sum_cols(const float* __restrict__ src, long MN, int ks, int nv, float (&acc)[4]) {
  int k = 0;
  for (; k + 4 <= ks; k += 4) {
    float x[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[u][r] = r < nv ? src[(long)(k + u) * MN + r] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += x[u][r];
  }
  for (; k < ks; ++k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += r < nv ? src[(long)k * MN + r] : 0.f;
  }
}

// split-K reduce of a GEMM with the FUSED BACKWARD epilogue (dX of a layer whose input has an
// activation; batch 1): v = act_bwd(bact, ay, act(alpha * sum + bias)), colsum[n] += sum over rows of v.
// Thread = 4 columns x RB rows: the column sums stay in registers, one atomic per (column, block),
// so small-batch dX GEMMs (summit_large: 256 x 4096 x 4096) can split K instead of running 64
// blocks of 128x128 tiles or 64x64 tiles at ~60 % of the big-tile rate.
// VEC: the host checked that every slab, ay and C quad is full and 16-B (bf16: 8-B) aligned; else the
// scalar form, which also serves a last quad that crosses N.
template <class P, bool VEC>
__global__ void __launch_bounds__(256) fm_gemm_reduce_bwd(P p, int RB) {
  const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (n >= p.N) return;
  const int m0 = blockIdx.y * RB, m1 = min(p.M, m0 + RB);
  const long MN = (long)p.M * p.N;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int m = m0; m < m1; ++m) {
    const float* src = p.ws + (long)m * p.N + n;
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (VEC) {
      const f32x4_t a = slab_sum4(src, MN, p.ksplit);
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[r] = a[r];
    } else {
      slab_sum_cols(src, MN, p.ksplit, p.N - n, sv);
    }
    gemm_out<4, false, true, VEC ? Q_VEC : Q_SCALAR>(p, 0, m, n, n + 3 < p.N, sv, cs);
  }
  if (p.colsum) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < p.N) atomicAdd(p.colsum + n + r, cs[r]);
  }
}

inline bool c_is_f32(const GemmP& p) { return p.c_fp32 != 0; }
inline bool c_is_f32(const GemmF&) { return true; }

// the reduce launch of a split-K GEMM (p.ksplit > 1); fused_bwd: it carries act_y / colsum
template <class P>
void launch_splitk_reduce(const P& p, bool fused_bwd, hipStream_t stream) {
  if (fused_bwd) {
    const int bx = (p.N + 1023) / 1024;
    const int by = std::max(1, std::min(p.M, 1024 / bx));
    const int RB = (p.M + by - 1) / by;
    const int cq = c_is_f32(p) ? 16 : 8;   // bytes of a quad of C
    const bool vec = ((p.N | p.ldc | (p.ay ? p.lday : 0)) & 3) == 0 && (((uintptr_t)p.C) & (cq - 1)) == 0 &&
                     (((uintptr_t)p.ay) & (4 * sizeof(*p.ay) - 1)) == 0;
    const dim3 grid(bx, (p.M + RB - 1) / RB);
    if (vec) hipLaunchKernelGGL((fm_gemm_reduce_bwd<P, true>), grid, dim3(256), 0, stream, p, RB);
    else hipLaunchKernelGGL((fm_gemm_reduce_bwd<P, false>), grid, dim3(256), 0, stream, p, RB);
    return;
  }
  const bool v4 = c_is_f32(p) && (p.N % 4 == 0) && (p.ldc % 4 == 0) && (p.sC % 4 == 0) && ((((uintptr_t)p.C) & 15) == 0);
  const long total = (long)p.M * p.N * p.batch / (v4 ? 4 : 1);
  if constexpr (P::kDeepReduce) {
    if (v4 && p.ksplit >= 16) {
      const dim3 grid((unsigned)((total + 256 / RD_G - 1) / (256 / RD_G)));
      if (p.uw) hipLaunchKernelGGL((fm_gemm_reduce_deep<P, true>), grid, dim3(256), 0, stream, p);
      else hipLaunchKernelGGL((fm_gemm_reduce_deep<P, false>), grid, dim3(256), 0, stream, p);
      return;
    }
  }
  const dim3 grid(fm_grid(total));
  if (p.uw) {
    if (v4) hipLaunchKernelGGL((fm_gemm_reduce<P, true, 4>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((fm_gemm_reduce<P, true, 1>), grid, dim3(256), 0, stream, p);
  } else {
    if (v4) hipLaunchKernelGGL((fm_gemm_reduce<P, false, 4>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((fm_gemm_reduce<P, false, 1>), grid, dim3(256), 0, stream, p);
  }
}

}  // namespace
