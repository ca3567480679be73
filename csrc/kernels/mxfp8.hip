// MXFP8 (OCP MX v1.0) for gfx950: block-scaled fp8 GEMM on v_mfma_scale_f32_16x16x128_f8f6f4 and the
// quantisers that feed it.  An MX tensor is fp8 codes (e4m3 = format 0, e5m2 = format 1) plus one E8M0
// byte per 32 consecutive elements of the contraction dimension: value = code * 2^(byte - 127).
//
// Operand layout of the instruction, measured on an MI355X (profiles/mxfp8.txt): lane l = 16 g + q holds
// row q of its operand; VGPRs 0..3 are k = 16 g .. 16 g + 15 and VGPRs 4..7 are k = 64 + 16 g .. 64 + 16 g + 15
// of the 128-deep step.  The scale of (row q, 32-block g) is byte `opsel` of the scale VGPR of lane 16 g + q,
// so a lane's 32 codes span two MX blocks, neither of them (for g = 1, 2) the one whose scale it carries.
// D[i][j] = sum_k A[i][k] B[j][k] lands as acc[r] = D[4 g + r][q].
//
//   fm_mx_quant       [R, C] bf16 / fp32 -> row-wise copy (codes [R, C], scales [R, C/32]) and / or
//                     column-wise copy (codes [C, Rp], scales [C, Rp/32], Rp = R rounded up to 128, pad = 0)
//   fm_mx_quant_dact  dpre = dy * act'(y) in fp32 -> both e5m2 copies, db += column sums (no atomics)
//   fm_mx_gemm        C[M, N] (+)= A[M, K] B[N, K]^T, K-contiguous codes, the output rule of gemm_epilogue.h
#include "gemm_epilogue.h"

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));

// ---- format --------------------------------------------------------------------------------------
// e = floor(log2 amax) - emax clamped to [-127, 127], from the exponent field (a zero or fp32-subnormal
// amax gives -127; flexmi/ops/mx.py does the same integer arithmetic)
template <int FMT>
FM_DEVICE int mx_exp(float amax) {
  const int e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - (FMT ? 15 : 8);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// 16 codes of v * 2^-e: the clamp to the format's maximum is explicit (the conversion instructions give
// NaN / inf past it), the rounding is the hardware's nearest-even with subnormals
template <int FMT>
FM_DEVICE u32x4_t mx_codes16(const float (&v)[16], int e) {
  const float mx = FMT ? 57344.f : 448.f;
  u32x4_t o;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = fminf(fmaxf(ldexpf(v[4 * w + j], -e), -mx), mx);
    int p = 0;
    if constexpr (FMT) {
      p = __builtin_amdgcn_cvt_pk_bf8_f32(s[0], s[1], p, false);
      p = __builtin_amdgcn_cvt_pk_bf8_f32(s[2], s[3], p, true);
    } else {
      p = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], p, false);
      p = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], p, true);
    }
    o[w] = (unsigned)p;
  }
  return o;
}

FM_DEVICE float amax16(const float (&v)[16]) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) a = fmaxf(a, fabsf(v[j]));
  return a;
}

// dy * act'(y) with the roundings of act_backward_torch (no contraction; the ReLU mask is a product, so
// a negative dy under a dead unit gives -0 as it does there)
FM_DEVICE float dact_exact(int act, float y, float dy) {
  if (act == ACT_RELU) return __fmul_rn(dy, y > 0.f ? 1.f : 0.f);
  if (act == ACT_SIGMOID) return __fmul_rn(__fmul_rn(dy, y), __fsub_rn(1.f, y));
  if (act == ACT_TANH) return __fmul_rn(dy, __fsub_rn(1.f, __fmul_rn(y, y)));
  return dy;
}

// ---- quantisers ------------------------------------------------------------------------------------
struct MxQuantP {
  const void* x; long ldx;       // the operand, or dy
  const void* y; long ldy;       // DACT: the activation output
  int act;
  long R; int C; long Rp;
  unsigned char* rc; unsigned char* rs;   // row-wise codes [R, C] and scales [R, C/32] (null: not wanted)
  unsigned char* cc; unsigned char* cs;   // column-wise codes [C, Rp] and scales [C, Rp/32]
  float* part;                   // DACT: column sums of every 32-row tile [tiles_r, C]
  int tiles_r, tiles_c;
};

template <class T>
FM_DEVICE void ld16(const T* p, float (&v)[16]) {
  float a[8], b[8];
  ld8<T>(p, a);
  ld8<T>(p + 8, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) { v[j] = a[j]; v[8 + j] = b[j]; }
}

// One wave per 32x32 tile.  Lane (r = lane / 2, h = lane % 2) reads 16 consecutive elements of row r:
// the row block's amax is one shuffle away, its 16 codes are one 16-B store.  The fp32 tile then goes
// through LDS (pitch 33) and the same lane takes 16 rows of column r: again one shuffle, one 16-B store
// into the transposed copy.  Rows past R read as zero, which writes the pad of the column-wise copy.
template <class T, int FMT, bool DACT>
__global__ __launch_bounds__(256) void mx_quant_kernel(MxQuantP p) {
  __shared__ float tile_s[4][32][33];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long tile = (long)blockIdx.x * 4 + wave;
  if (tile >= (long)p.tiles_r * p.tiles_c) return;   // whole waves leave; nothing below is block-wide
  const int tr = (int)(tile / p.tiles_c), tc = (int)(tile % p.tiles_c);
  const int r = lane >> 1, h = lane & 1;
  const long row = (long)tr * 32 + r;
  const int col = tc * 32 + 16 * h;
  float v[16];
  if (row < p.R) {
    ld16<T>(reinterpret_cast<const T*>(p.x) + row * p.ldx + col, v);
    if constexpr (DACT) {
      float yv[16];
      ld16<T>(reinterpret_cast<const T*>(p.y) + row * p.ldy + col, yv);
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = dact_exact(p.act, yv[j], v[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = 0.f;
  }
  const int nbr = p.C / 32;
  if (p.rc && row < p.R) {
    float am = amax16(v);
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    const int e = mx_exp<FMT>(am);
    *reinterpret_cast<u32x4_t*>(p.rc + row * p.C + col) = mx_codes16<FMT>(v, e);
    if (h == 0) p.rs[row * nbr + tc] = (unsigned char)(e + 127);
  }
  if (!p.cc && !DACT) return;
  float(*ts)[33] = tile_s[wave];
#pragma unroll
  for (int j = 0; j < 16; ++j) ts[r][16 * h + j] = v[j];
  FM_WAVE_LDS_SYNC();
  float t[16];   // column r of the tile, rows 16 h .. 16 h + 15
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = ts[16 * h + j][r];
  const long ccol = (long)tc * 32 + r;
  if (p.cc) {
    float am = amax16(t);
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    const int e = mx_exp<FMT>(am);
    *reinterpret_cast<u32x4_t*>(p.cc + ccol * p.Rp + (long)tr * 32 + 16 * h) = mx_codes16<FMT>(t, e);
    if (h == 0) p.cs[ccol * (p.Rp / 32) + tr] = (unsigned char)(e + 127);
  }
  if constexpr (DACT) {
    if (p.part) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += t[j];
      s += __shfl_xor(s, 1, 64);
      if (h == 0) p.part[(long)tr * p.C + ccol] = s;
    }
  }
}

// db[c] += sum over the row tiles of part[t][c], in tile order
__global__ void mx_colsum_fold_kernel(const float* __restrict__ part, float* __restrict__ db, int C, int tiles) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  db[c] += slab_sum1(part + c, C, tiles);
}

template <class T, bool DACT>
void mx_quant_launch(const MxQuantP& p, int fmt, hipStream_t s) {
  const long tiles = (long)p.tiles_r * p.tiles_c;
  const dim3 grid((unsigned)((tiles + 3) / 4));
  if (fmt) hipLaunchKernelGGL((mx_quant_kernel<T, 1, DACT>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((mx_quant_kernel<T, 0, DACT>), grid, dim3(256), 0, s, p);
}

// ---- GEMM ------------------------------------------------------------------------------------------
// C[M, N] (+)= A[M, K] B[N, K]^T.  B rows are the MFMA's first operand and A rows its second, so that a
// lane ends up with four consecutive columns of one output row: the layout gemm_out stores.
struct MxGemmP {
  GemmP g;   // the output rule's fields (M, N, K, bias, act, beta, C, ldc, c_fp32, tile order)
  const unsigned char* A; const unsigned char* sa; long lda, ldsa;
  const unsigned char* B; const unsigned char* sb; long ldb, ldsb;
};

constexpr int MX_BM = 128, MX_BN = 128, MX_BK = 128;   // block tile; MX_BK bytes = one MFMA step
constexpr int MX_IMG = MX_BM * MX_BK;                  // one operand image: 16 KiB

// Four 16-B chunks per thread and operand: chunk t % 8 of rows t / 8 + 32 i, zero past the edges
FM_DEVICE void mx_stage_load(const unsigned char* src, long ld, int rows, int K, int row0, int k0, int tid, u32x4_t (&reg)[4]) {
  const int c = tid & 7, r0 = tid >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + r0 + 32 * i, k = k0 + 16 * c;
    reg[i] = (row < rows && k < K) ? *reinterpret_cast<const u32x4_t*>(src + (long)row * ld + k) : u32x4_t{0u, 0u, 0u, 0u};
  }
}
FM_DEVICE void mx_stage_store(char* img, int tid, const u32x4_t (&reg)[4]) {
  const int c = tid & 7, r0 = tid >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4_t*>(img + lds_off<true, 0>(r0 + 32 * i, c)) = reg[i];
}

// the operand of lane (q, g) for the 16 rows from `base`: chunks g and 4 + g of row base + q
FM_DEVICE i32x8_t mx_frag(const char* img, int base, int q, int g) {
  const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(img + lds_off<true, 0>(base + q, g));
  const u32x4_t hi = *reinterpret_cast<const u32x4_t*>(img + lds_off<true, 0>(base + q, 4 + g));
  i32x8_t f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[j] = (int)lo[j]; f[4 + j] = (int)hi[j]; }
  return f;
}

// the scale bytes lane (q, g) carries for its four 16-row tiles: (row base + 16 i + q, block kb + g).
// Rows past the edge take the last row's byte and blocks past K take 127: their codes are zero.
FM_DEVICE void mx_scales(const unsigned char* s, long lds, int rows, int nblk, int base, int blk, int (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(base + 16 * i, rows - 1);
    out[i] = blk < nblk ? (int)s[(long)row * lds + blk] : 127;
  }
}

template <int FA, int FB>
__global__ __launch_bounds__(256) void mx_gemm_kernel(MxGemmP p) {
  __shared__ __attribute__((aligned(16))) char lds[4 * MX_IMG];   // [buffer][A image, B image]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const TileMN tl = tile_coords(p.g, xcd_remap(blockIdx.x, p.g.tiles_m * p.g.tiles_n));
  const int m0 = tl.m * MX_BM, n0 = tl.n * MX_BN;
  const int M = p.g.M, N = p.g.N, K = p.g.K, nblk = K / 32, nk = (K + MX_BK - 1) / MX_BK;

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  u32x4_t ra[4], rb[4];
  int sca[4], scb[4], sca_n[4], scb_n[4];
  mx_stage_load(p.A, p.lda, M, K, m0, 0, tid, ra);
  mx_stage_load(p.B, p.ldb, N, K, n0, 0, tid, rb);
  mx_scales(p.sa, p.ldsa, M, nblk, m0 + wm * 64 + q, g, sca_n);
  mx_scales(p.sb, p.ldsb, N, nblk, n0 + wn * 64 + q, g, scb_n);
  mx_stage_store(lds, tid, ra);
  mx_stage_store(lds + MX_IMG, tid, rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const char* ia = lds + (kt & 1) * 2 * MX_IMG;
    const char* ib = ia + MX_IMG;
#pragma unroll
    for (int i = 0; i < 4; ++i) { sca[i] = sca_n[i]; scb[i] = scb_n[i]; }
    const bool more = kt + 1 < nk;
    if (more) {   // the next step's operands and scales travel while this one computes
      mx_stage_load(p.A, p.lda, M, K, m0, (kt + 1) * MX_BK, tid, ra);
      mx_stage_load(p.B, p.ldb, N, K, n0, (kt + 1) * MX_BK, tid, rb);
      mx_scales(p.sa, p.ldsa, M, nblk, m0 + wm * 64 + q, 4 * (kt + 1) + g, sca_n);
      mx_scales(p.sb, p.ldsb, N, nblk, n0 + wn * 64 + q, 4 * (kt + 1) + g, scb_n);
    }
    i32x8_t fa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = mx_frag(ia, wm * 64 + 16 * i, q, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x8_t fb = mx_frag(ib, wn * 64 + 16 * j, q, g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa[i], acc[i][j], FB, FA, 0, scb[j], 0, sca[i]);
    }
    if (more) {
      char* na = lds + ((kt + 1) & 1) * 2 * MX_IMG;
      mx_stage_store(na, tid, ra);
      mx_stage_store(na + MX_IMG, tid, rb);
    }
    __syncthreads();
  }

  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + 16 * i + q;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + 16 * j + 4 * g;
      if (n >= N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      gemm_out<4, false, false>(p.g, 0, m, n, n + 4 <= N, v, cs);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int fm_mx_quant(const void* x, long ldx, int bf16, long R, int C, int fmt, void* rc, void* rs, void* cc,
                           void* cs, long Rp, hipStream_t s) {
  const int eb = bf16 ? 2 : 4;
  if (R < 1 || C < 32 || C % 32 || (fmt != 0 && fmt != 1) || (!rc && !cc) || !aligned16(x) || (ldx * eb) % 16 ||
      ldx < C || !aligned16(rc) || !aligned16(cc) || (cc && (Rp % 128 || Rp < R)))
    return 1;
  MxQuantP p{};
  p.x = x; p.ldx = ldx; p.R = R; p.C = C; p.Rp = Rp;
  p.rc = (unsigned char*)rc; p.rs = (unsigned char*)rs; p.cc = (unsigned char*)cc; p.cs = (unsigned char*)cs;
  p.tiles_r = (int)((cc ? Rp : R + 31) / 32);
  p.tiles_c = C / 32;
  if (bf16) mx_quant_launch<unsigned short, false>(p, fmt, s);
  else mx_quant_launch<float, false>(p, fmt, s);
  return 0;
}

extern "C" long fm_mx_dact_ws_bytes(long R, int C) { return ((R + 127) / 128 * 4) * (long)C * 4; }

extern "C" int fm_mx_quant_dact(const void* dy, long lddy, const void* y, long ldy, int bf16, int act, long R, int C,
                                void* rc, void* rs, void* cc, void* cs, long Rp, float* db, float* ws, long ws_bytes,
                                hipStream_t s) {
  const int eb = bf16 ? 2 : 4;
  if (R < 1 || C < 32 || C % 32 || !rc || !cc || !aligned16(dy) || !aligned16(y) || (lddy * eb) % 16 || (ldy * eb) % 16 ||
      lddy < C || ldy < C || !aligned16(rc) || !aligned16(cc) || Rp % 128 || Rp < R)
    return 1;
  if (db && (!ws || ws_bytes < fm_mx_dact_ws_bytes(R, C))) return 2;
  MxQuantP p{};
  p.x = dy; p.ldx = lddy; p.y = y; p.ldy = ldy; p.act = act; p.R = R; p.C = C; p.Rp = Rp;
  p.rc = (unsigned char*)rc; p.rs = (unsigned char*)rs; p.cc = (unsigned char*)cc; p.cs = (unsigned char*)cs;
  p.part = db ? ws : nullptr;
  p.tiles_r = (int)(Rp / 32);
  p.tiles_c = C / 32;
  if (bf16) mx_quant_launch<unsigned short, true>(p, 1, s);
  else mx_quant_launch<float, true>(p, 1, s);
  if (db) hipLaunchKernelGGL(mx_colsum_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, ws, db, C, p.tiles_r);
  return 0;
}

extern "C" int fm_mx_gemm(const void* A, long lda, const void* sa, long ldsa, int fmt_a, const void* B, long ldb,
                          const void* sb, long ldsb, int fmt_b, void* C, long ldc, int c_fp32, const float* bias, int act,
                          int beta, int M, int N, int K, hipStream_t s) {
  if (M < 1 || N < 1 || K < 32 || K % 32 || fmt_b != 0 || (fmt_a != 0 && fmt_a != 1) || !aligned16(A) || !aligned16(B) ||
      lda % 16 || ldb % 16 || lda < K || ldb < K || ldsa < K / 32 || ldsb < K / 32 || ldc < N)
    return 1;
  MxGemmP p{};
  p.A = (const unsigned char*)A; p.sa = (const unsigned char*)sa; p.lda = lda; p.ldsa = ldsa;
  p.B = (const unsigned char*)B; p.sb = (const unsigned char*)sb; p.ldb = ldb; p.ldsb = ldsb;
  p.g.C = C; p.g.ldc = ldc; p.g.c_fp32 = c_fp32; p.g.bias = bias; p.g.act = act; p.g.beta = beta; p.g.alpha = 1.f;
  p.g.M = M; p.g.N = N; p.g.K = K; p.g.ksplit = 1; p.g.batch = 1; p.g.bact = ACT_NONE;
  p.g.tiles_m = (M + MX_BM - 1) / MX_BM;
  p.g.tiles_n = (N + MX_BN - 1) / MX_BN;
  p.g.n_fast = M >= N;   // the smaller operand's tiles change fastest: the larger one's row block stays in L2
  const dim3 grid((unsigned)(p.g.tiles_m * p.g.tiles_n));
  if (fmt_a) hipLaunchKernelGGL((mx_gemm_kernel<1, 0>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((mx_gemm_kernel<0, 0>), grid, dim3(256), 0, s, p);
  return 0;
}
