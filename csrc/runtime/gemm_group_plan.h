// Host-side plan of a grouped split-K GEMM launch (csrc/kernels/gemm_f32.hip fm_gemm_f32_grouped):
// several small-grid problems on 256x128 tiles share one grid, problem g running tiles_g * ks_g blocks.
// Plain C++ with no GPU dependency, so the CPU-only runtime module binds it too (tests).
//
// A 256x128 split-bf16 block costs about 17 us + 0.0745 us per k (profiles/gemm_tune_candidates_r6.jsonl),
// one block per CU: a problem with 16-32 tiles launched alone splits K 8- or 16-fold to fill the chip
// and pays the fixed part each time; problems that fill it together at a shallower depth pay it once.
#pragma once

namespace flexmi {

constexpr int kGemmGroupMax = 4;
constexpr int kGemmGroupBM = 256, kGemmGroupBN = 128, kGemmGroupBK = 32;

// One member of fm_gemm_f32_grouped (csrc/kernels/gemm_f32.hip; the binding in csrc/bindings/hip_ops.cpp
// fills it): C = (beta ? C : 0) + A B, rowsum_a[m] += sum_k A(m, k) when given (MN-contiguous A).
struct GemmGroupItem {
  const float* A; long lda;
  const float* B; long ldb;
  float* C; long ldc;
  float* rowsum_a;
  int M, N, K, beta;
};

struct GemmGroupPlan {
  int n = 0;
  int tiles[kGemmGroupMax];        // output tiles of problem g
  int ks[kGemmGroupMax];           // its split-K depth (1: the tiles store C themselves, no slabs)
  int first[kGemmGroupMax + 1];    // its first flat block id; first[n] = the grid
  long ws_off[kGemmGroupMax];      // byte offset of its slabs [ks][M][N] in the workspace (16-B aligned)
  long ws_bytes = 0;               // workspace bytes the group uses
};

// Where flat block id `bid` of the grid works: problem g, and in it tile (in the problem's own launch
// order) and k split, the tile fastest.  The kernels compute exactly this.
inline void gemm_group_locate(const GemmGroupPlan& pl, int bid, int& g, int& tile, int& split) {
  g = 0;
  for (int i = 1; i < pl.n; ++i) g += bid >= pl.first[i];
  const int lb = bid - pl.first[g];
  tile = lb % pl.tiles[g];
  split = lb / pl.tiles[g];
}

// Plans n problems (M x N outputs, K deep, K % 32 == 0) for a device of `cus` compute units and a
// workspace of `ws_bytes`.  force > 0: every problem at that depth (at most its k steps), as a forced
// single-GEMM configuration would run it.  Otherwise the largest depths with sum tiles_g * ks_g <= cus,
// each at most ktiles_g / 4 and 16: first the largest common power of two, then single problems doubled
// while they fit (widest first).  False = not grouped: fewer than two problems or more than
// kGemmGroupMax, the tiles alone fill the device, no common depth above 1 fits, or the slabs exceed
// the workspace.
inline bool gemm_group_plan(const int* M, const int* N, const int* K, int n, int cus, long ws_bytes, int force,
                            GemmGroupPlan& pl) {
  if (n < 2 || n > kGemmGroupMax || cus <= 0) return false;
  pl.n = n;
  long sum_tiles = 0;
  int cap[kGemmGroupMax];
  for (int g = 0; g < n; ++g) {
    if (M[g] <= 0 || N[g] <= 0 || K[g] <= 0 || K[g] % kGemmGroupBK != 0) return false;
    pl.tiles[g] = ((M[g] + kGemmGroupBM - 1) / kGemmGroupBM) * ((N[g] + kGemmGroupBN - 1) / kGemmGroupBN);
    const int ktiles = K[g] / kGemmGroupBK;
    cap[g] = force > 0 ? (force < ktiles ? force : ktiles) : (ktiles / 4 < 16 ? ktiles / 4 : 16);
    if (cap[g] < 1) cap[g] = 1;
    sum_tiles += pl.tiles[g];
  }
  if (sum_tiles >= cus) return false;
  auto blocks = [&]() {
    long b = 0;
    for (int g = 0; g < n; ++g) b += (long)pl.tiles[g] * pl.ks[g];
    return b;
  };
  if (force > 0) {
    for (int g = 0; g < n; ++g) pl.ks[g] = cap[g];
  } else {
    int ks = 1;
    for (;;) {
      long b = 0;
      bool grows = false;
      for (int g = 0; g < n; ++g) {
        const int k2 = 2 * ks < cap[g] ? 2 * ks : cap[g];
        grows = grows || k2 > (ks < cap[g] ? ks : cap[g]);
        b += (long)pl.tiles[g] * k2;
      }
      if (!grows || b > cus) break;
      ks *= 2;
    }
    if (ks < 2) return false;
    for (int g = 0; g < n; ++g) pl.ks[g] = ks < cap[g] ? ks : cap[g];
    for (bool any = true; any;) {   // what is left of the device: widest problem first
      any = false;
      int best = -1;
      for (int g = 0; g < n; ++g)
        if (2 * pl.ks[g] <= cap[g] && blocks() + (long)pl.tiles[g] * pl.ks[g] <= cus &&
            (best < 0 || pl.tiles[g] > pl.tiles[best]))
          best = g;
      if (best >= 0) {
        pl.ks[best] *= 2;
        any = true;
      }
    }
  }
  long off = 0;
  pl.first[0] = 0;
  for (int g = 0; g < n; ++g) {
    pl.first[g + 1] = pl.first[g] + pl.tiles[g] * pl.ks[g];
    pl.ws_off[g] = off;
    if (pl.ks[g] > 1) off += ((long)pl.ks[g] * M[g] * N[g] * 4 + 15) & ~15L;
  }
  pl.ws_bytes = off;
  return off <= ws_bytes;
}

}  // namespace flexmi
