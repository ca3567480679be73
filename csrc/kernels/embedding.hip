// Embedding-bag kernels (replace src/ops/embedding.cu:173-224 embed_forward / embed_backward, which
// ran one thread per (sample, column) with the bag loop inside and one launch per table).
//
// All kernels take a TABLE DESCRIPTOR ARRAY and process every table of an embedding group in ONE
// launch (blockIdx.y = table) -- the executor fuses the independent per-table Embedding ops of a
// DLRM graph (26 ops in the MLPerf config) into one forward and two backward launches.
// The index width (int32/int64) is a template parameter and every load in the hot loops is
// unconditional (clamped address, predicated use): a runtime width test or a guarded load makes
// the compiler emit a branch + s_waitcnt vmcnt(0) per load, i.e. one HBM round trip per sample
// (measured 3-8x slowdowns before this rule was applied).
//
// Forward: lane = 4 consecutive columns of one sample (D/4 lanes per row: a 512-B fp32 row of a
// D=128 table is read by 32 lanes with 16-B loads), sum over the bag, bf16/fp32 output written
// with 8/16-B stores straight into the consumer's buffer (row stride ldo).  Five forms
// (fm_embedding_fwd_last_form names the one a launch set ran): tables of one bag size get the same
// grid each (blockIdx.y = table) -- fm_emb_fwd_multi, whose single-lookup bags take emb_bal_short
// ("multi_su"), fm_emb_fwd_split for long bags on small batches, fm_emb_fwd_multi_scalar for
// D % 4 != 0; tables of unequal bag sizes (per-table multi-hot sizes) share a one-dimensional grid
// dealt out by lookups -- "work-balanced forward" below.
// Backward (fused sparse SGD: W[idx] -= lr*scale*dy; or dense-grad accumulate when lr == null):
//   * mostly-unique tables with claim buffers: owner-computes (claim / dup / owner kernels), plain
//     16-B read-modify-writes of the touched rows instead of row atomics;
//   * regular tables: one wave-instruction = 64 consecutive fp32 atomic adds (256 contiguous bytes:
//     the full gfx950 atomic rate, MI355X_MICROARCH "Global float atomics");
//   * tiny tables (<= 64 rows: 3, 4, 10, 14, 36, 63 rows in the MLPerf set): thousands of samples hit the
//     same few addresses, which L2 serialises; each wave accumulates into a PRIVATE LDS copy of the
//     table gradient with plain read-add-write (row index wave-uniform, lane = column: 64 distinct
//     banks, no atomics), the block sums its waves' copies and flushes one atomic per (row, col).
// Backward under Adagrad (tables that are not replicated): the sparse-DP coalesce (claim / assign /
// dups) sums the duplicate lookups of a row, then fm_emb_adagrad_apply updates the accumulator and
// the weights of the touched rows only -- see "fused sparse Adagrad" below; row-wise Adagrad keeps
// one accumulator per row and also takes replicated tables -- "fused sparse row-wise Adagrad".
// Said once and shared: the lane-group map (lane_map_vec / lane_map_scalar, host mirrors rpi_vec /
// rpi_scalar), the four-wide output store (emb_store4), gradient load (emb_grad4) and gather-sum
// (emb_gather_sum), and on the host the launch-set loop (for_each_batch / for_each_width_batch)
// and the (element type, index width) dispatch (with_types).
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int MAXT = 32;

// Row-sharded tables (SOAP row split of the embedding weight): a shard holds the global rows
// [lo, lo + rows); lookups outside it contribute nothing here (their partial sums come from the
// shards that hold them).  Whole tables have lo = 0, and out-of-range indices are dropped, never
// read or written out of bounds.  The range test is a select AFTER an unconditional (clamped)
// load, so the hot loops keep their branch-free loads.
struct TabDesc {
  const float* W;     // fwd: table (read); bwd: table or dense grad (written)
  const void* idx;    // [B, bag] int32/int64
  void* act;          // fwd: out [B, *] (row stride ld); bwd: dy
  long ld;
  long lo;            // first global row held by this shard
  int rows, D, bag;   // rows: rows held by this shard
  float scale;
};

// local row of a lookup, clamped into the shard (ok = the shard holds it)
FM_DEVICE long local_row(long r, long lo, int rows, bool& ok) {
  const long l = r - lo;
  ok = (unsigned long)l < (unsigned long)rows;
  return ok ? l : 0;
}
struct TabSet {
  TabDesc t[MAXT];
  int n;
};

template <bool I64>
FM_DEVICE long ldi(const void* p, long i) {
  if constexpr (I64) return (long)reinterpret_cast<const long long*>(p)[i];
  else return (long)reinterpret_cast<const int*>(p)[i];
}

// Lane-group map: the 256 threads of a block form rpi groups of lpr lanes, one group per row (a
// sample, a lookup or a payload row).  sub = this thread's group, lc = its lane in the group; the
// threads left over when lpr does not divide 256 are not live.
struct LaneMap {
  int lpr, rpi, sub, lc;
  bool live;
};
FM_DEVICE LaneMap lane_map(int want, int cap) {
  LaneMap m;
  m.lpr = want < cap ? want : cap;
  m.rpi = 256 / m.lpr;
  m.sub = threadIdx.x / m.lpr;
  m.lc = threadIdx.x - m.sub * m.lpr;
  m.live = m.sub < m.rpi;
  return m;
}
// vector form: a lane owns 4 consecutive columns (one 16-B access), at most 64 lanes per row
FM_DEVICE LaneMap lane_map_vec(int D) { return lane_map(D >> 2, 64); }
// scalar form: a lane owns a column, at most 256 lanes per row
FM_DEVICE LaneMap lane_map_scalar(int D) { return lane_map(D, 256); }
// the host's mirrors: rows per block-iteration of a table of D columns
inline int rpi_vec(int D) { return 256 / std::min(64, std::max(1, D / 4)); }
inline int rpi_scalar(int D) { return 256 / std::min(256, std::max(1, D)); }

template <typename OutT>
FM_DEVICE void emb_store4(OutT* o, const f32x4_t acc) {
  if constexpr (sizeof(OutT) == 4) {
    *reinterpret_cast<f32x4_t*>(o) = acc;
  } else {
    bf16x4_t w;
    w[0] = (short)f2bf(acc[0]); w[1] = (short)f2bf(acc[1]); w[2] = (short)f2bf(acc[2]); w[3] = (short)f2bf(acc[3]);
    *reinterpret_cast<bf16x4_t*>(o) = w;
  }
}

// four consecutive gradients (bf16: one 8-B load, fp32: one 16-B load) as fp32
template <typename GT>
FM_DEVICE f32x4_t emb_grad4(const GT* p) {
  if constexpr (sizeof(GT) == 2) {
    const bf16x4_t g = *reinterpret_cast<const bf16x4_t*>(p);
    return f32x4_t{bf2f((unsigned short)g[0]), bf2f((unsigned short)g[1]), bf2f((unsigned short)g[2]),
                   bf2f((unsigned short)g[3])};
  } else {
    return *reinterpret_cast<const f32x4_t*>(p);
  }
}

// acc + the rows of lookup entries e0, e0 + stride, ..., e0 + (U - 1) * stride at columns [c, c + 4):
// U index loads, then U row loads in flight per lane (instead of one dependent index -> row round
// trip per lookup), then the adds in ascending order, each predicated on its shard holding the row.
// acc goes in and out by value: by reference the eight-wide instance took 2 more VGPRs.
template <bool I64, int U>
FM_DEVICE f32x4_t emb_gather_sum(const TabDesc& d, long e0, int stride, int c, f32x4_t acc) {
  long r[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) r[u] = local_row(ldi<I64>(d.idx, e0 + u * stride), d.lo, d.rows, ok[u]);
  f32x4_t v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const f32x4_t*>(d.W + r[u] * d.D + c);
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (ok[u]) acc += v[u];
  return acc;
}

// bags of at most U lookups: S samples' index loads, then their S * U row loads in flight per lane
template <typename OutT, bool I64, int S, int U>
FM_DEVICE void emb_bal_short(const TabDesc& d, long B, long b_first, long bstride, int c) {
  for (long b0 = b_first; b0 < B; b0 += S * bstride) {
    long r[S][U];
    bool ok[S][U];
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const long e0 = min(b0 + q * bstride, B - 1) * d.bag;
#pragma unroll
      for (int u = 0; u < U; ++u) r[q][u] = local_row(ldi<I64>(d.idx, e0 + min(u, d.bag - 1)), d.lo, d.rows, ok[q][u]);
    }
    f32x4_t v[S][U];
#pragma unroll
    for (int q = 0; q < S; ++q)
#pragma unroll
      for (int u = 0; u < U; ++u) v[q][u] = *reinterpret_cast<const f32x4_t*>(d.W + r[q][u] * d.D + c);
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const long b = b0 + q * bstride;
      if (b >= B) break;
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (u < d.bag && ok[q][u]) acc += v[q][u];
      acc *= d.scale;
      emb_store4<OutT>(reinterpret_cast<OutT*>(d.act) + b * d.ld + c, acc);
    }
  }
}

template <typename OutT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_fwd_multi(TabSet s, long B) {
  const TabDesc& d = s.t[blockIdx.y];
  const LaneMap m = lane_map_vec(d.D);
  if (!m.live) return;
  const int D4 = d.D >> 2;
  const long bstride = (long)gridDim.x * m.rpi, b_first = (long)blockIdx.x * m.rpi + m.sub;
  // the bag loop stands first and the single-lookup call last: the other way round the compiler
  // spends 4 more VGPRs on the bag loop (profiles/embedding_refactor_device_diff.txt)
  if (d.bag != 1 || D4 > 64) {
    for (long b = b_first; b < B; b += bstride) {
      for (int c4 = m.lc; c4 < D4; c4 += m.lpr) {
        const int c = c4 * 4;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        int j = 0;
        // long bags (summit_large: 100 lookups per sample, 256 samples): eight lookups at a time
        for (; j + 8 <= d.bag; j += 8) acc = emb_gather_sum<I64, 8>(d, b * d.bag + j, 1, c, acc);
        for (; j < d.bag; ++j) acc = emb_gather_sum<I64, 1>(d, b * d.bag + j, 0, c, acc);
        acc *= d.scale;
        emb_store4<OutT>(reinterpret_cast<OutT*>(d.act) + b * d.ld + c, acc);
      }
    }
    return;
  }
  // one lookup per sample (the MLPerf tables): four samples' index loads, then their row loads in
  // flight per lane, so a small grid still streams at the HBM rate and leaves CU slots to the
  // bottom-MLP GEMMs running beside it on the other stream
  emb_bal_short<OutT, I64, 4, 1>(d, B, b_first, bstride, m.lc * 4);
}

// Long bags on small batches (summit_large: 256 samples x 100 lookups per table): one lane group
// per sample leaves ~100 blocks for 256 CUs, each lane walking the whole bag.  Here SP lane groups
// share a sample -- group k sums lookups k, k+SP, ... -- and the block folds the SP partial rows
// through LDS.  D <= 256 (one 16-B column chunk per lane, lpr = D/4 lanes per row).
template <typename OutT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_fwd_split(TabSet s, long B, int sp) {
  __shared__ f32x4_t part[256];
  const TabDesc& d = s.t[blockIdx.y];
  const LaneMap m = lane_map_vec(d.D);             // rpi lane groups per block
  const int spb = m.rpi / sp;                      // samples per block
  const bool live = m.sub < spb * sp;              // whole sample groups only
  const int si = m.sub / sp, k = m.sub - si * sp;
  const long b = (long)blockIdx.x * spb + si;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  if (live && b < B) {
    const int c = m.lc * 4;
    int j = k;
    for (; j + 3 * sp < d.bag; j += 4 * sp) acc = emb_gather_sum<I64, 4>(d, b * d.bag + j, sp, c, acc);
    for (; j < d.bag; j += sp) acc = emb_gather_sum<I64, 1>(d, b * d.bag + j, 0, c, acc);
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (!live || k != 0 || b >= B) return;
  for (int q = 1; q < sp; ++q) acc += part[threadIdx.x + q * m.lpr];
  acc *= d.scale;
  emb_store4<OutT>(reinterpret_cast<OutT*>(d.act) + b * d.ld + m.lc * 4, acc);
}

// scalar fallback for D % 4 != 0 (any D)
template <typename OutT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_fwd_multi_scalar(TabSet s, long B) {
  const TabDesc& d = s.t[blockIdx.y];
  const LaneMap m = lane_map_scalar(d.D);
  if (!m.live) return;
  for (long b = (long)blockIdx.x * m.rpi + m.sub; b < B; b += (long)gridDim.x * m.rpi)
    for (int c = m.lc; c < d.D; c += m.lpr) {
      float acc = 0.f;
      for (int j = 0; j < d.bag; ++j) {
        bool ok;
        const long r = local_row(ldi<I64>(d.idx, b * d.bag + j), d.lo, d.rows, ok);
        const float v = d.W[r * d.D + c];
        if (ok) acc += v;
      }
      st<OutT>(reinterpret_cast<OutT*>(d.act) + b * d.ld + c, acc * d.scale);
    }
}

// ---- work-balanced forward for tables of UNEQUAL bag sizes (per-table multi-hot sizes) --------
// fm_emb_fwd_multi gives every table the same grid; with the MLPerf multi-hot sizes (1..100
// lookups per sample, 214 in all) the bag-100 table does 47 % of the row reads on 1/26 of the
// blocks.  Here the grid is one dimension and the host deals the blocks out in proportion to each
// table's lookups (first[i] = first block of table i); a block finds its table by a wave-uniform
// scan of first[], then strides over that table's samples with its local id and that table's
// block count.  lpr / rpi are per table, so tables of different D share a launch.  The sums run in
// ascending bag order with the arithmetic and the stores of fm_emb_fwd_multi: the outputs are equal
// bit for bit.  Every load is unconditional at a clamped address (see the header).
struct BalSet {
  TabDesc t[MAXT];
  int first[MAXT + 1];
  int n;
};

template <typename OutT, bool I64, int U>
__global__ void __launch_bounds__(256) fm_emb_fwd_balanced(BalSet s, long B) {
  const int bid = blockIdx.x;
  int ti = 0;
  for (int i = 1; i < s.n; ++i) ti += bid >= s.first[i];      // first[] ascends: wave-uniform scan
  const TabDesc& d = s.t[ti];
  const int lb = bid - s.first[ti], nb = s.first[ti + 1] - s.first[ti];
  const LaneMap m = lane_map_vec(d.D);             // D <= 256: one 16-B column chunk per lane
  if (!m.live) return;
  const int c = m.lc * 4;
  const long bstride = (long)nb * m.rpi, b_first = (long)lb * m.rpi + m.sub;
  if (d.bag == 1) return emb_bal_short<OutT, I64, 4, 1>(d, B, b_first, bstride, c);
  if (d.bag <= 4) return emb_bal_short<OutT, I64, 2, 4>(d, B, b_first, bstride, c);
  // longer bags in chunks of U: the chunk's U row loads and the NEXT chunk's U index loads are in
  // flight together, so a chunk costs one round trip, not an index trip and then a row trip
  for (long b = b_first; b < B; b += bstride) {
    const long e0 = b * d.bag;
    long r[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = local_row(ldi<I64>(d.idx, e0 + min(u, d.bag - 1)), d.lo, d.rows, ok[u]);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < d.bag; j += U) {
      f32x4_t v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const f32x4_t*>(d.W + r[u] * d.D + c);
      bool okc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        okc[u] = ok[u];
        r[u] = local_row(ldi<I64>(d.idx, e0 + min(j + U + u, d.bag - 1)), d.lo, d.rows, ok[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j + u < d.bag && okc[u]) acc += v[u];
    }
    acc *= d.scale;
    emb_store4<OutT>(reinterpret_cast<OutT*>(d.act) + b * d.ld + c, acc);
  }
}

template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_bwd_atomic_multi(TabSet s, const float* __restrict__ lr, long B) {
  const TabDesc& d = s.t[blockIdx.y];
  const float mul = (lr ? -lr[0] : 1.f) * d.scale;
  const LaneMap m = lane_map_scalar(d.D);
  if (!m.live) return;
  float* W = const_cast<float*>(d.W);
  const GT* dy = reinterpret_cast<const GT*>(d.act);
  for (long b = (long)blockIdx.x * m.rpi + m.sub; b < B; b += (long)gridDim.x * m.rpi) {
    bool ok0;
    const long r0 = local_row(ldi<I64>(d.idx, b * d.bag), d.lo, d.rows, ok0);
    for (int c = m.lc; c < d.D; c += m.lpr) {
      const float g = ld<GT>(dy + b * d.ld + c) * mul;
      if (ok0) atomicAdd(W + r0 * d.D + c, g);
      for (int j = 1; j < d.bag; ++j) {
        bool ok;
        const long r = local_row(ldi<I64>(d.idx, b * d.bag + j), d.lo, d.rows, ok);
        if (ok) atomicAdd(W + r * d.D + c, g);
      }
    }
  }
}

template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_bwd_tiny_multi(TabSet s, const float* __restrict__ lr, long B, int chunk) {
  constexpr int S = 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);     // [4][rows*D]
  const TabDesc& d = s.t[blockIdx.y];
  const long b0 = (long)blockIdx.x * chunk;
  if (b0 >= B) return;
  const long b1 = min(B, b0 + chunk);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = d.rows * d.D;
  float* mine = red + wave * n;
  for (int i = lane; i < n; i += 64) mine[i] = 0.f;
  const GT* dy = reinterpret_cast<const GT*>(d.act);
  for (long bw = b0 + (long)wave * S; bw < b1; bw += 4L * S) {
    for (int c0 = 0; c0 < d.D; c0 += 128) {
      const int ca = c0 + lane, cb = c0 + 64 + lane;
      const int sa = min(ca, d.D - 1), sb = min(cb, d.D - 1);   // clamped: loads stay unconditional
      long r[S];
      bool rok[S];
      float ga[S], gb[S];
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const long bu = min(bw + u, b1 - 1);
        r[u] = local_row(ldi<I64>(d.idx, bu * d.bag), d.lo, d.rows, rok[u]);
        ga[u] = ld<GT>(dy + bu * d.ld + sa);
        gb[u] = ld<GT>(dy + bu * d.ld + sb);
      }
#pragma unroll
      for (int u = 0; u < S; ++u) {
        if (bw + u >= b1) break;                       // wave-uniform
        float* p = mine + r[u] * d.D;
        if (rok[u] && ca < d.D) p[ca] += ga[u];
        if (rok[u] && cb < d.D) p[cb] += gb[u];
        for (int j = 1; j < d.bag; ++j) {              // further bag entries share the gradient row
          bool ok;
          float* q = mine + local_row(ldi<I64>(d.idx, (bw + u) * d.bag + j), d.lo, d.rows, ok) * d.D;
          if (ok && ca < d.D) q[ca] += ga[u];
          if (ok && cb < d.D) q[cb] += gb[u];
        }
      }
    }
  }
  __syncthreads();
  const float mul = (lr ? -lr[0] : 1.f) * d.scale;
  float* W = const_cast<float*>(d.W);
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = red[i] + red[n + i] + red[2 * n + i] + red[3 * n + i];
    if (v != 0.f) atomicAdd(W + i, v * mul);
  }
}

// ---- host helpers -------------------------------------------------------------------------------
// The tables k < n that take(k) accepts, cut into launch sets of at most MAXT: fn(ks, m) gets the
// table numbers ks[0 .. m) of one set.
template <typename Take, typename Fn>
void for_each_batch(int n, Take take, Fn fn) {
  std::vector<int> sel;
  for (int k = 0; k < n; ++k)
    if (take(k)) sel.push_back(k);
  for (size_t base = 0; base < sel.size(); base += MAXT)
    fn(sel.data() + base, (int)std::min<size_t>(MAXT, sel.size() - base));
}
// the same per index width (the width is a template parameter of the kernels, so a launch set holds
// one width): int32 tables first, then int64; fn(ks, m, wide)
template <typename Take, typename Fn>
void for_each_width_batch(int n, const int* idx64, Take take, Fn fn) {
  for (int w = 0; w < 2; ++w) {
    const bool wide = w != 0;
    for_each_batch(n, [&](int k) { return (idx64[k] != 0) == wide && take(k); },
                   [&](const int* ks, int m) { fn(ks, m, wide); });
  }
}
inline bool every_table(int) { return true; }

// (bf16?, int64?) -> template arguments: fn gets a value whose type names the activation / gradient
// element type (T::elem) and the index width (T::wide)
template <typename E, bool W>
struct EmbTypes {
  using elem = E;
  static constexpr bool wide = W;
};
template <typename Fn>
void with_types(bool bf16, bool wide, Fn fn) {
  if (bf16 && wide) fn(EmbTypes<unsigned short, true>{});
  else if (bf16) fn(EmbTypes<unsigned short, false>{});
  else if (wide) fn(EmbTypes<float, true>{});
  else fn(EmbTypes<float, false>{});
}

// fm_embedding_set_fwd_mode: 0 = auto (balanced for vectorisable sets of unequal bags), 1 = never
// balanced, 2 = balanced for every vectorisable set.  Auto takes the balanced kernel because it
// measured 226 -> 171 us (fp32 out) and 200 -> 154 us (bf16 out) on the 26 MLPerf multi-hot tables at
// B = 8192 (224 -> 181 and 218 -> 169 us in a second session); on tiny_dcn_multihot's four tables,
// which are launch-bound, it is 0.2-0.5 us slower (3.5-3.8 -> 4.0 us).
int g_emb_fwd_mode = 0;
// the chunk of the balanced kernel's bag loop: of U = 2 / 4 / 8 at 1 / 2 / 4 x the block budget, U = 2
// at x1 measured fastest, by 1-4 % over U = 4 (profiles/emb_fwd_multihot_ab.txt; the others are deleted)
constexpr int BAL_U = 2;
// which kernel this thread's last forward launch set ran (fm_embedding_fwd_last_form)
enum FwdForm { FWD_NONE = 0, FWD_MULTI, FWD_MULTI_SU, FWD_SPLIT, FWD_SCALAR, FWD_BALANCED };
thread_local int g_emb_fwd_form = FWD_NONE;

// Block shares: the budget is the grid fm_emb_fwd_multi would launch (so the forward takes the same
// share of the chip beside the bottom-MLP GEMMs); table i gets blocks in proportion to its lookups
// B * bag_i, at least one and at most one per rows-per-iteration of its samples.
template <typename OutT, bool I64>
void launch_balanced(const TabSet& s, int m, long B, long budget, hipStream_t st) {
  BalSet bs;
  long sumbag = 0;
  for (int i = 0; i < m; ++i) sumbag += s.t[i].bag;
  bs.first[0] = 0;
  for (int i = 0; i < m; ++i) {
    bs.t[i] = s.t[i];
    const int rpi = rpi_vec(s.t[i].D);
    const long cap = (B + rpi - 1) / rpi;
    const long want = (budget * s.t[i].bag + sumbag / 2) / sumbag;
    bs.first[i + 1] = bs.first[i] + (int)std::max<long>(1, std::min(want, cap));
  }
  for (int i = m + 1; i <= MAXT; ++i) bs.first[i] = bs.first[m];
  bs.n = m;
  const dim3 grid((unsigned)bs.first[m]);
  hipLaunchKernelGGL((fm_emb_fwd_balanced<OutT, I64, BAL_U>), grid, dim3(256), 0, st, bs, B);
}

template <typename OutT, bool I64>
void launch_fwd(const TabSet& s, int m, bool vec, long B, int D0, hipStream_t st) {
  const int rpi = rpi_vec(D0);
  bool uniform = true;
  for (int i = 1; i < m; ++i) uniform = uniform && s.t[i].bag == s.t[0].bag;
  if (vec && (g_emb_fwd_mode == 2 || (g_emb_fwd_mode == 0 && !uniform))) {
    const long budget = std::max<long>(1, std::min<long>((B + rpi - 1) / rpi, 256L)) * m;
    launch_balanced<OutT, I64>(s, m, B, budget, st);
    g_emb_fwd_form = FWD_BALANCED;
    return;
  }
  // long bags with too few samples to fill the chip: split every bag over SP lane groups
  // (measured on summit_large, profiles/README.md)
  int minbag = 1 << 30, maxD = 0, minD = 1 << 30;
  for (int i = 0; i < m; ++i) {
    minbag = std::min(minbag, s.t[i].bag);
    maxD = std::max(maxD, s.t[i].D);
    minD = std::min(minD, s.t[i].D);
  }
  if (vec && maxD == minD && maxD <= 256 && minbag >= 16 && (B + rpi - 1) / rpi * m < 1024) {
    int sp = 1;
    while (sp * 2 <= rpi && sp * 2 <= minbag / 4 && (B * sp * 2 + rpi - 1) / rpi * m <= 2048) sp *= 2;
    if (sp > 1) {
      const int spb = rpi / sp;
      dim3 grid((unsigned)((B + spb - 1) / spb), m);
      hipLaunchKernelGGL((fm_emb_fwd_split<OutT, I64>), grid, dim3(256), 0, st, s, B, sp);
      g_emb_fwd_form = FWD_SPLIT;
      return;
    }
  }
  // 256 blocks per table: the forward runs beside the bottom MLP on a second stream; fewer,
  // longer-running blocks leave CUs to its GEMMs: MLPerf fp32 step 1.181 ms at 2048 blocks per
  // table, 1.164 at 256, 1.172 at 64 (profiles/bench_ab_x3_sched_embgrid_r5n.txt).  Single-lookup
  // bags take four samples per lane-group iteration (emb_bal_short<.., 4, 1>;
  // profiles/bench_ab_emb_fwd_su_r5zc.txt)
  dim3 grid((unsigned)std::max<long>(1, std::min<long>((B + rpi - 1) / rpi, 256L)), m);
  if (vec) {
    hipLaunchKernelGGL((fm_emb_fwd_multi<OutT, I64>), grid, dim3(256), 0, st, s, B);
    g_emb_fwd_form = uniform && s.t[0].bag == 1 ? FWD_MULTI_SU : FWD_MULTI;   // su: the single-lookup loop
  } else {
    g_emb_fwd_form = FWD_SCALAR;
    hipLaunchKernelGGL((fm_emb_fwd_multi_scalar<OutT, I64>), grid, dim3(256), 0, st, s, B);
  }
}

// ---- mostly-unique tables (rows > B*bag): owner-computes sparse SGD without row atomics -------
// claim: every lookup entry e CASes its row's owner slot (-1 -> e); the winner owns the row, the
// others are appended to a per-table duplicate list.  dup: one wave per duplicate adds its row
// update with float atomics (few for large tables).  owner (after dup, kernel boundary): each
// owner does a plain 16-B read-modify-write of its row and releases the claim (-1), so the table
// is touched with full-line stores at the HBM rate instead of the ~1.3 TB/s atomic rate.
struct ClaimDesc {
  float* W;
  const void* idx;
  const void* dy;
  long ld;
  long lo;
  int rows, D, bag;
  float scale;
  int* owner;   // [rows] int32, -1 = free (restored by the owner kernel)
  int* dups;    // [B*bag]
  int* ndup;    // [1]
};
struct ClaimSet {
  ClaimDesc t[MAXT];
  int n;
};

template <bool I64>
__global__ void __launch_bounds__(256) fm_emb_claim_multi(ClaimSet s, long B) {
  const ClaimDesc& d = s.t[blockIdx.y];
  const long n = B * d.bag;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    bool ok;
    const long r = local_row(ldi<I64>(d.idx, e), d.lo, d.rows, ok);
    if (!ok) continue;                               // row held by another shard
    const int prev = atomicCAS(d.owner + r, -1, (int)e);
    if (prev != -1) d.dups[atomicAdd(d.ndup, 1)] = (int)e;
  }
}

template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_dup_multi(ClaimSet s, const float* __restrict__ lr) {
  const ClaimDesc& d = s.t[blockIdx.y];
  const int nd = *d.ndup;
  const float mul = -lr[0] * d.scale;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const GT* dy = reinterpret_cast<const GT*>(d.dy);
  for (long k = blockIdx.x * 4L + wave; k < nd; k += (long)gridDim.x * 4) {
    const long e = d.dups[k];
    const long b = e / d.bag, r = ldi<I64>(d.idx, e) - d.lo;   // dups hold in-shard entries only
    for (int c = lane; c < d.D; c += 64) atomicAdd(d.W + r * d.D + c, ld<GT>(dy + b * d.ld + c) * mul);
  }
}

template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_emb_owner_multi(ClaimSet s, const float* __restrict__ lr, long B) {
  const ClaimDesc& d = s.t[blockIdx.y];
  const float mul = -lr[0] * d.scale;
  const LaneMap m = lane_map_vec(d.D);
  const int D4 = d.D >> 2;
  const long n = B * d.bag;
  const GT* dy = reinterpret_cast<const GT*>(d.dy);
  if (m.live) {
    for (long e = (long)blockIdx.x * m.rpi + m.sub; e < n; e += (long)gridDim.x * m.rpi) {
      bool ok;
      const long r = local_row(ldi<I64>(d.idx, e), d.lo, d.rows, ok);
      if (!ok || d.owner[r] != (int)e) continue;   // uniform across the row's lanes
      const long b = e / d.bag;
      for (int c4 = m.lc; c4 < D4; c4 += m.lpr) {
        const int c = c4 * 4;
        f32x4_t* wp = reinterpret_cast<f32x4_t*>(d.W + r * d.D + c);
        f32x4_t w = *wp;
        w += mul * emb_grad4<GT>(dy + b * d.ld + c);
        *wp = w;
      }
      if (m.lc == 0) d.owner[r] = -1;                // release the claim for the next step
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *d.ndup = 0;   // the dup kernel has finished reading it
}

// the grid-stride backward kernels (claim / dup / owner / atomic) take their full grids, up to the
// caps below
template <typename GT, bool I64>
void launch_claim(const ClaimSet& s, int m, const float* lr, long B, int maxbag, int minD, hipStream_t st) {
  const long n = B * maxbag;
  dim3 gc((unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 1024)), m);
  hipLaunchKernelGGL((fm_emb_claim_multi<I64>), gc, dim3(256), 0, st, s, B);
  // (a 64-block grid measured 18.4 vs 9.5 us/step: 12k..40k-row tables still see thousands of dups)
  dim3 gd((unsigned)std::max<long>(1, std::min<long>((n + 3) / 4, 1024)), m);
  hipLaunchKernelGGL((fm_emb_dup_multi<GT, I64>), gd, dim3(256), 0, st, s, lr);
  const int rpi = rpi_vec(minD);
  dim3 go((unsigned)std::max<long>(1, std::min<long>((n + rpi - 1) / rpi, 2048)), m);
  hipLaunchKernelGGL((fm_emb_owner_multi<GT, I64>), go, dim3(256), 0, st, s, lr, B);
}

template <typename GT, bool I64>
void launch_bwd(const TabSet& s, int m, bool tiny, const float* lr, long B, int maxD, hipStream_t st) {
  if (tiny) {
    size_t lds = 0;
    for (int i = 0; i < m; ++i) lds = std::max(lds, (size_t)s.t[i].rows * s.t[i].D * 4 * 4);  // one copy per wave
    static bool attr = false;
    if (!attr) {   // > 64 KiB of dynamic LDS (above 32 rows at D = 128) needs the opt-in
      (void)hipFuncSetAttribute((const void*)fm_emb_bwd_tiny_multi<GT, I64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 << 10);
      attr = true;
    }
    // 64-sample chunks keep the per-wave chain to one round trip; at large B more blocks would
    // pile onto the same few addresses in the flush (tools/bench_embedding.py: B=8192 -> 64,
    // B=65536 -> 128..256)
    const int chunk = B <= 16384 ? 64 : B <= 32768 ? 128 : 256;
    dim3 grid((unsigned)((B + chunk - 1) / chunk), m);
    hipLaunchKernelGGL((fm_emb_bwd_tiny_multi<GT, I64>), grid, dim3(256), lds, st, s, lr, B, chunk);
  } else {
    const int rpi = rpi_scalar(maxD);
    dim3 grid((unsigned)std::max<long>(1, std::min<long>((B + rpi - 1) / rpi, 2048)), m);
    hipLaunchKernelGGL((fm_emb_bwd_atomic_multi<GT, I64>), grid, dim3(256), 0, st, s, lr, B);
  }
}

// ---- sparse data parallelism for replicated tables ---------------------------------------------
// A table replicated over R ranks (DP on its sample dim) is trained WITHOUT a dense gradient: each
// replica coalesces its own lookups into (unique local row, summed gradient) pairs, the replica set
// all-gathers those payloads, and every replica applies the R segments in rank order -- the same
// fp32 operations in the same order everywhere, so the replicas stay bit-identical.  Within one
// segment the rows are unique: the apply is a plain read-modify-write, no atomics.
//   claim  : every in-shard lookup e CASes its row's slot (-1 -> e)
//   assign : the winner takes a compact id u (one atomic per unique row), writes cid[e] = u,
//            ids[u] = row and g[u] = scale * dy[b] with plain stores
//   dups   : every other lookup of the row atomically adds its gradient into g[cid[slot[row]]]
//   apply  : per segment r: W[ids[u]] -= lr * g[u] for u < count; the own segment also frees the
//            slots (slot = -1) and zeroes its count for the next step
struct SdpDesc {
  const void* idx;    // [B, bag] int32/int64 (global rows)
  const void* dy;     // [B, *] bf16/fp32, row stride ld
  long ld;
  long lo;            // first global row of this shard
  int rows, D, bag;
  float scale;
  int* slot;          // [rows] int32, -1 = free
  int* cid;           // [B*bag] compact id of an owner entry (scratch)
  int* ids;           // [nmax] unique local rows      (payload)
  float* g;           // [nmax][D] summed gradients   (payload)
  int* count;         // [1] unique rows              (payload)
};
struct SdpSet {
  SdpDesc t[MAXT];
  int n;
};

template <bool I64>
__global__ void __launch_bounds__(256) fm_sdp_claim(SdpSet s, long B) {
  const SdpDesc& d = s.t[blockIdx.y];
  const long n = B * d.bag;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    bool ok;
    const long r = local_row(ldi<I64>(d.idx, e), d.lo, d.rows, ok);
    if (ok) atomicCAS(d.slot + r, -1, (int)e);
  }
}

// one wave per lookup entry (lane = column): the row's owner entry takes the compact id
template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_sdp_assign(SdpSet s, long B) {
  const SdpDesc& d = s.t[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long n = B * d.bag;
  const GT* dy = reinterpret_cast<const GT*>(d.dy);
  for (long e = blockIdx.x * 4L + wave; e < n; e += (long)gridDim.x * 4) {
    bool ok;
    const long r = local_row(ldi<I64>(d.idx, e), d.lo, d.rows, ok);
    if (!ok || d.slot[r] != (int)e) continue;       // wave-uniform
    int u = 0;
    if (lane == 0) u = atomicAdd(d.count, 1);
    u = __shfl(u, 0, 64);
    const long b = e / d.bag;
    float* gu = d.g + (long)u * d.D;
    for (int c = lane; c < d.D; c += 64) gu[c] = ld<GT>(dy + b * d.ld + c) * d.scale;
    if (lane == 0) {
      d.ids[u] = (int)r;
      d.cid[e] = u;
    }
  }
}

template <typename GT, bool I64>
__global__ void __launch_bounds__(256) fm_sdp_dups(SdpSet s, long B) {
  const SdpDesc& d = s.t[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long n = B * d.bag;
  const GT* dy = reinterpret_cast<const GT*>(d.dy);
  for (long e = blockIdx.x * 4L + wave; e < n; e += (long)gridDim.x * 4) {
    bool ok;
    const long r = local_row(ldi<I64>(d.idx, e), d.lo, d.rows, ok);
    if (!ok) continue;
    const int own = d.slot[r];
    if (own == (int)e) continue;                     // the owner entry wrote g[u] itself
    const long b = e / d.bag;
    float* gu = d.g + (long)d.cid[own] * d.D;
    for (int c = lane; c < d.D; c += 64) atomicAdd(gu + c, ld<GT>(dy + b * d.ld + c) * d.scale);
  }
}

// one segment of the gathered payloads: W[ids[u]] -= lr * g[u] (rows unique within a segment)
struct SdpApply {
  float* W;
  const int* ids;
  const float* g;
  const int* count;
  int D;
  int* slot;          // own segment: free the claimed slots; else nullptr
  int* own_count;     // own segment: this rank's count, zeroed after use; else nullptr
};
struct SdpApplySet {
  SdpApply t[MAXT];
  int n;
};

__global__ void __launch_bounds__(256) fm_sdp_apply(SdpApplySet s, const float* __restrict__ lr, int nmax) {
  const SdpApply& d = s.t[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cnt = min(*d.count, nmax);
  const float mlr = -lr[0];
  for (long u = blockIdx.x * 4L + wave; u < cnt; u += (long)gridDim.x * 4) {
    const long r = d.ids[u];
    float* w = d.W + r * d.D;
    const float* gu = d.g + u * d.D;
    for (int c = lane; c < d.D; c += 64) w[c] += mlr * gu[c];
    if (d.slot && lane == 0) d.slot[r] = -1;
  }
}

// zero per-table counts once the launches before it on the stream have read them (a separate tiny
// launch of MAXT threads or more: the sparse-DP own segment's count may be read by later segments'
// launches only through the gathered copy); null entries are skipped
struct CountSet {
  int* c[MAXT] = {};
};
__global__ void fm_emb_zero_counts(CountSet s) {
  if (threadIdx.x < MAXT && s.c[threadIdx.x]) *s.c[threadIdx.x] = 0;
}

// ---- fused sparse Adagrad for non-replicated tables ---------------------------------------------
// The coalesce above (claim / assign / dups) leaves one payload per table: count unique local rows
// ids[u] with their summed gradients g[u].  Element-wise Adagrad of the touched rows only,
//   H[r] += g g;  W[r] -= lr g / (sqrt(H[r]) + eps)      (r = ids[u], u < count),
// equals dense Adagrad: an untouched row has gradient 0 and keeps H and W (no weight decay here).
// Rows are unique within a payload, so H and W take plain read-modify-writes, no atomics.  The
// count is read on the device (no host sync; capturable).  D % 4 == 0: D/4 lanes per row with
// 16-B accesses (D = 128: 32 lanes, two rows per wave) and two rows in flight per lane -- the
// second one's address is clamped to the last payload row and only its stores are predicated, so
// the loads of an iteration stay unconditional.  Other D: one wave per row, lane = column.
// (Row-wise Adagrad -- one accumulator per row -- is a different optimizer: see below.  Both apply
// kernels take this descriptor.)
struct AdaDesc {
  float* W;           // [rows][D] table shard
  float* H;           // accumulator: [rows][D] (element-wise) or [rows] (row-wise)
  const int* ids;     // [nmax] unique local rows      (payload)
  const float* g;     // [nmax][D] summed gradients   (payload)
  int* count;         // [1] unique rows; zeroed by fm_emb_zero_counts after the apply
  int* slot;          // [rows] claim slots, freed (-1) here
  int D, nmax, vec;
};
struct AdaSet {
  AdaDesc t[MAXT];
  int n;
};

__global__ void __launch_bounds__(256) fm_emb_adagrad_apply_multi(AdaSet s, const float* __restrict__ lr_p, float eps) {
  const AdaDesc& d = s.t[blockIdx.y];
  const long cnt = min(*d.count, d.nmax);
  if (cnt <= 0) return;
  const float lr = lr_p[0];
  if (d.vec) {
    const LaneMap m = lane_map_vec(d.D);
    if (!m.live) return;
    const int D4 = d.D >> 2, lc = m.lc;
    const long stride = (long)gridDim.x * m.rpi;
    for (long u0 = (long)blockIdx.x * m.rpi + m.sub; u0 < cnt; u0 += 2 * stride) {
      const bool live1 = u0 + stride < cnt;            // uniform across the row's lanes
      const long u1 = live1 ? u0 + stride : cnt - 1;
      const long r0 = d.ids[u0], r1 = d.ids[u1];
      for (int c4 = lc; c4 < D4; c4 += m.lpr) {
        const int c = c4 * 4;
        f32x4_t* hp0 = reinterpret_cast<f32x4_t*>(d.H + r0 * d.D + c);
        f32x4_t* wp0 = reinterpret_cast<f32x4_t*>(d.W + r0 * d.D + c);
        f32x4_t* hp1 = reinterpret_cast<f32x4_t*>(d.H + r1 * d.D + c);
        f32x4_t* wp1 = reinterpret_cast<f32x4_t*>(d.W + r1 * d.D + c);
        const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(d.g + u0 * d.D + c);
        const f32x4_t g1 = *reinterpret_cast<const f32x4_t*>(d.g + u1 * d.D + c);
        f32x4_t h0 = *hp0, h1 = *hp1, w0 = *wp0, w1 = *wp1;
        h0 += g0 * g0;
        h1 += g1 * g1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          w0[j] -= lr * g0[j] / (sqrtf(h0[j]) + eps);
          w1[j] -= lr * g1[j] / (sqrtf(h1[j]) + eps);
        }
        *hp0 = h0;
        *wp0 = w0;
        if (live1) {
          *hp1 = h1;
          *wp1 = w1;
        }
      }
      if (lc == 0) {
        d.slot[r0] = -1;                               // release the claims for the next step
        if (live1) d.slot[r1] = -1;
      }
    }
  } else {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long u = blockIdx.x * 4L + wave; u < cnt; u += (long)gridDim.x * 4) {
      const long r = d.ids[u];
      float* h = d.H + r * d.D;
      float* w = d.W + r * d.D;
      const float* gu = d.g + u * d.D;
      for (int c = lane; c < d.D; c += 64) {
        const float g = gu[c];
        const float hc = h[c] + g * g;
        h[c] = hc;
        w[c] -= lr * g / (sqrtf(hc) + eps);
      }
      if (lane == 0) d.slot[r] = -1;
    }
  }
}

// ---- fused sparse row-wise Adagrad ---------------------------------------------------------------
// One fp32 accumulator per table row ("exact row-wise Adagrad"), applied to a coalesced payload:
//   h[r] += (1/D) sum_c g[u][c]^2;  W[r][c] -= lr g[u][c] / (sqrt(h[r]) + eps)     (r = ids[u], u < count)
// Per touched row the kernel reads g once and read-modify-writes W: 3 D words against the 5 D of
// the element-wise form.  D % 4 == 0: D/4 lanes own a row with 16-B accesses; the lane group is
// the next power of two (at most 64, surplus lanes idle: D = 48 -> 12 of 16 lanes), so a row's sum
// of squares is an xor butterfly inside the wave -- no LDS, no atomics, and every lane of the
// group ends with the same bits.  The row's g stays in registers between the sum and the W update;
// above D = 256 a lane takes several 16-B chunks, sums them first and re-reads g for the update.
// Other D: one wave per row, lane = column.  The outer loop runs the same number of times in every
// lane of the block (the shuffles need whole waves): a group past the payload's end works on the
// clamped last row with its stores predicated off.  One row is in flight per lane group: a second,
// clamped row as in the element-wise kernel measured slower (39.9 vs 36.0 us,
// profiles/emb_rowwise_adagrad_ab.txt).  One lane writes h[r] and frees slot[r].  The summation order depends on D alone, so replicas that
// apply the same payload values stay bit-identical.
__device__ inline float sumsq4(const f32x4_t v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }

__global__ void __launch_bounds__(256) fm_emb_rowwise_apply_multi(AdaSet s, const float* __restrict__ lr_p, float eps) {
  const AdaDesc& d = s.t[blockIdx.y];                  // d.H: [rows], one accumulator per row
  const long cnt = min(*d.count, d.nmax);
  if (cnt <= 0) return;                                // uniform across the block
  const float lr = lr_p[0];
  const float invD = 1.0f / (float)d.D;
  if (d.vec) {
    const int D4 = d.D >> 2;
    const int act = D4 < 64 ? D4 : 64;                 // lanes of a group that hold columns
    int G = 1;
    while (G < act) G <<= 1;                           // the group: a power of two, 1..64
    const int rpi = 256 / G;
    const int sub = threadIdx.x / G, lc = threadIdx.x & (G - 1);
    const bool col = lc < act;
    const int c0 = (col ? lc : 0) * 4;                 // idle lanes load column 0 and drop it
    for (long base = (long)blockIdx.x * rpi; base < cnt; base += (long)gridDim.x * rpi) {
      const bool live = base + sub < cnt;              // uniform across the row's lanes
      const long u = live ? base + sub : cnt - 1;
      const long r = d.ids[u];
      const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(d.g + u * d.D + c0);
      const f32x4_t w = *reinterpret_cast<const f32x4_t*>(d.W + r * d.D + c0);
      const float hv = d.H[r];
      float ss = col ? sumsq4(gv) : 0.0f;
      for (int c4 = lc + 64; c4 < D4; c4 += 64)        // D > 256: further chunks of this lane
        ss += sumsq4(*reinterpret_cast<const f32x4_t*>(d.g + u * d.D + c4 * 4));
      for (int off = G >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
      const float hn = hv + ss * invD;
      const float mul = lr / (sqrtf(hn) + eps);
      if (live && col) {
        *reinterpret_cast<f32x4_t*>(d.W + r * d.D + c0) = w - mul * gv;
        for (int c4 = lc + 64; c4 < D4; c4 += 64) {
          f32x4_t* wp = reinterpret_cast<f32x4_t*>(d.W + r * d.D + c4 * 4);
          *wp = *wp - mul * *reinterpret_cast<const f32x4_t*>(d.g + u * d.D + c4 * 4);
        }
      }
      if (live && lc == 0) {
        d.H[r] = hn;
        d.slot[r] = -1;                                // release the claim for the next step
      }
    }
  } else {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long u = blockIdx.x * 4L + wave; u < cnt; u += (long)gridDim.x * 4) {   // uniform across the wave
      const long r = d.ids[u];
      float* w = d.W + r * d.D;
      const float* gu = d.g + u * d.D;
      float ss = 0.0f;
      for (int c = lane; c < d.D; c += 64) ss += gu[c] * gu[c];
      for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
      const float hn = d.H[r] + ss * invD;
      const float mul = lr / (sqrtf(hn) + eps);
      for (int c = lane; c < d.D; c += 64) w[c] -= mul * gu[c];
      if (lane == 0) {
        d.H[r] = hn;
        d.slot[r] = -1;
      }
    }
  }
}

// ---- replicated tables under row-wise Adagrad: deterministic merge of the gathered segments ------
// Applying the R segments one after another (fm_sdp_apply) would square each replica's gradient
// on its own; Adagrad needs the replicas' gradients of a row summed first.  Per step, after the
// pack and the all-gather:
//   release : free the own claim slots (they hold lookup indices after the coalesce) and zero the
//             own count;
//   merge   : one launch per segment in replica-rank order.  A row not seen yet takes a merged
//             index m (one integer atomic on the merged count), records slot[r] = m, mids[m] = r
//             and STORES its gradient; a row seen in an earlier segment ADDS into mg[slot[r]] with
//             a plain read-modify-write (rows are unique within a segment and the launches are
//             ordered on the stream -- no float atomics).  Every row's sum is formed in rank order
//             on every replica: m may differ between replicas, the values may not;
//   apply   : fm_emb_rowwise_adagrad_apply on (mids, mg, mcount); it frees the slots and zeroes the
//             merged count.
struct RwMerge {
  const int* ids;     // [nmax] this segment's unique local rows
  const float* g;     // [nmax][D] their gradients
  const int* count;   // [1]
  int* slot;          // [rows] -1 = not seen this step, else the merged index
  int* mids;          // [mcap] merged rows
  float* mg;          // [mcap][D] merged gradients
  int* mcount;        // [1] merged rows so far
  int rows, D, nmax, mcap, vec;
};
struct RwMergeSet {
  RwMerge t[MAXT];
  int n;
};
struct RwRelease {
  const int* ids;     // own payload
  int* count;         // own count, zeroed by fm_emb_zero_counts after the release
  int* slot;
  int rows, nmax;
};
struct RwReleaseSet {
  RwRelease t[MAXT];
  int n;
};

__global__ void __launch_bounds__(256) fm_sdp_rowwise_release(RwReleaseSet s) {
  const RwRelease& d = s.t[blockIdx.y];
  const long cnt = min(*d.count, d.nmax);
  for (long u = blockIdx.x * 256L + threadIdx.x; u < cnt; u += (long)gridDim.x * 256) {
    const int r = d.ids[u];
    if ((unsigned)r < (unsigned)d.rows) d.slot[r] = -1;
  }
}

// one wave per segment row (lane = 16-B chunk, or column in the scalar form)
__global__ void __launch_bounds__(256) fm_sdp_rowwise_merge(RwMergeSet s) {
  const RwMerge& d = s.t[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long cnt = min(*d.count, d.nmax);
  for (long u = blockIdx.x * 4L + wave; u < cnt; u += (long)gridDim.x * 4) {     // uniform across the wave
    const int r = d.ids[u];
    if ((unsigned)r >= (unsigned)d.rows) continue;
    int m = 0;
    if (lane == 0) {
      m = d.slot[r];
      if (m < 0) {
        m = atomicAdd(d.mcount, 1);
        if (m < d.mcap) {
          d.slot[r] = m;
          d.mids[m] = r;
        }
        m = ~m;                                        // negative: a first sight, the row is stored
      }
    }
    m = __shfl(m, 0, 64);
    const bool first = m < 0;
    if (first) m = ~m;
    if (m >= d.mcap) continue;                         // cannot happen: mcap = min(rows, R * nmax)
    const float* gu = d.g + u * d.D;
    float* mo = d.mg + (long)m * d.D;
    if (d.vec) {
      for (int c4 = lane; c4 < (d.D >> 2); c4 += 64) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(gu + c4 * 4);
        f32x4_t* mp = reinterpret_cast<f32x4_t*>(mo + c4 * 4);
        *mp = first ? v : *mp + v;
      }
    } else {
      for (int c = lane; c < d.D; c += 64) mo[c] = first ? gu[c] : mo[c] + gu[c];
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Launchers.  Arrays describe n tables; act/ld = outputs (fwd) or output grads (bwd).  Tables
// are batched by index width (and, in backward, by kernel: owner-computes, tiny, atomic) into launches of <= 32 tables.
// lo: first global row of each table shard (nullptr = whole tables); rows: rows held
extern "C" void fm_embedding_fwd_multi(int n, const float* const* W, const void* const* idx, const int* idx64,
                                       void* const* out, const long* ldo, const long* lo, const int* rows, const int* D,
                                       const int* bag, const float* scale, int out_bf16, long B, hipStream_t st) {
  if (B <= 0) return;
  for_each_width_batch(n, idx64, every_table, [&](const int* ks, int m, bool wide) {
    TabSet s;
    bool vec = true;
    for (int i = 0; i < m; ++i) {
      const int k = ks[i];
      s.t[i] = TabDesc{W[k], idx[k], out[k], ldo[k], lo ? lo[k] : 0, rows[k], D[k], bag[k], scale[k]};
      vec = vec && (D[k] % 4 == 0) && (ldo[k] % 4 == 0) && D[k] <= 256;
    }
    s.n = m;
    with_types(out_bf16 != 0, wide, [&](auto t) {
      launch_fwd<typename decltype(t)::elem, decltype(t)::wide>(s, m, vec, B, D[ks[0]], st);
    });
  });
}

extern "C" void fm_embedding_set_fwd_mode(int mode) { g_emb_fwd_mode = mode == 1 || mode == 2 ? mode : 0; }
// out[0] = the form of this thread's last forward launch set: 0 none, 1 multi, 2 multi_su, 3 split,
// 4 scalar, 5 balanced
extern "C" void fm_embedding_fwd_last_form(int* out) { out[0] = g_emb_fwd_form; }

// lr != nullptr: fused sparse SGD into W; lr == nullptr: W is a dense grad buffer (accumulate).
extern "C" void fm_embedding_bwd_multi(int n, float* const* W, const void* const* idx, const int* idx64,
                                       const void* const* dy, const long* ldg, const long* lo, const int* rows, const int* D,
                                       const int* bag, const float* scale, int dy_bf16, const float* lr, long B,
                                       int* const* owner, int* const* dups, int* const* ndup, hipStream_t st) {
  if (B <= 0) return;
  // owner-computes path: fused SGD, claim buffers given, 16-B rows
  auto claimable = [&](int k) {
    return lr != nullptr && owner != nullptr && owner[k] != nullptr && D[k] % 4 == 0 && ldg[k] % 4 == 0 &&
           D[k] <= 256;
  };
  for_each_width_batch(n, idx64, claimable, [&](const int* ks, int m, bool wide) {
    ClaimSet s;
    int maxbag = 1, minD = 256;
    for (int i = 0; i < m; ++i) {
      const int k = ks[i];
      s.t[i] = ClaimDesc{W[k], idx[k], dy[k], ldg[k], lo ? lo[k] : 0, rows[k], D[k], bag[k], scale[k], owner[k], dups[k],
                         ndup[k]};
      maxbag = std::max(maxbag, bag[k]);
      minD = std::min(minD, D[k]);
    }
    s.n = m;
    with_types(dy_bf16 != 0, wide, [&](auto t) {
      launch_claim<typename decltype(t)::elem, decltype(t)::wide>(s, m, lr, B, maxbag, minD, st);
    });
  });
  // the other tables: tiny (wave-private LDS copies) or regular (atomics).  Measured and deleted in
  // r6: a block-shared LDS copy for 36..155-row tables (113 vs 16.6 us of regular atomics) and
  // row-block ownership for <= 8192-row tables (76 vs 48 us; profiles/emb_bwd_rowblock_r5u.jsonl)
  auto tiny = [&](int k) {
    // the wave-private LDS kernel up to tiny_rows rows while its four copies fit the LDS (rows * D *
    // 16 B).  64 takes the 36- and 63-row MLPerf tables off the same-address atomics: slower alone
    // (35.5 vs 32.3 us for the eight <= 155-row tables) but less contention beside the bottom-MLP
    // backward, step 1.145-1.164 vs 1.170-1.173 ms at 16 (profiles/emb_tiny_rows_ab_r5tr.txt).  A
    // block-shared copy with LDS float atomics for <= 160 rows measured 93.5 vs 30.5 us (r7, removed).
    constexpr int tiny_rows = 64;
    return rows[k] <= tiny_rows && (long)rows[k] * D[k] * 16 <= (160L << 10) && D[k] <= 256 &&
           B * (long)bag[k] >= 16L * rows[k];
  };
  for (const bool want_tiny : {true, false}) {
    for_each_width_batch(n, idx64, [&](int k) { return !claimable(k) && tiny(k) == want_tiny; },
                         [&](const int* ks, int m, bool wide) {
      TabSet s;
      int maxD = 1;
      for (int i = 0; i < m; ++i) {
        const int k = ks[i];
        s.t[i] = TabDesc{W[k], idx[k], const_cast<void*>(dy[k]), ldg[k], lo ? lo[k] : 0, rows[k], D[k], bag[k], scale[k]};
        maxD = std::max(maxD, D[k]);
      }
      s.n = m;
      with_types(dy_bf16 != 0, wide, [&](auto t) {
        launch_bwd<typename decltype(t)::elem, decltype(t)::wide>(s, m, want_tiny, lr, B, maxD, st);
      });
    });
  }
}

// single-table conveniences
extern "C" void fm_embedding_fwd(const void* idx, int idx64, const float* W, void* out, int out_bf16, long B, int bag,
                                 int rows, int D, long ldo, float scale, hipStream_t s) {
  fm_embedding_fwd_multi(1, &W, &idx, &idx64, &out, &ldo, nullptr, &rows, &D, &bag, &scale, out_bf16, B, s);
}

extern "C" void fm_embedding_bwd(const void* idx, int idx64, const void* dy, int dy_bf16, float* W, const float* lr,
                                 long B, int bag, int rows, int D, long ldg, float scale, hipStream_t s) {
  fm_embedding_bwd_multi(1, &W, &idx, &idx64, &dy, &ldg, nullptr, &rows, &D, &bag, &scale, dy_bf16, lr, B, nullptr,
                         nullptr, nullptr, s);
}

// ---- sparse DP launchers -------------------------------------------------------------------
template <typename GT, bool I64>
static void launch_coalesce(const SdpSet& s, dim3 gc, dim3 gw, long B, hipStream_t st) {
  hipLaunchKernelGGL((fm_sdp_claim<I64>), gc, dim3(256), 0, st, s, B);
  hipLaunchKernelGGL((fm_sdp_assign<GT, I64>), gw, dim3(256), 0, st, s, B);
  hipLaunchKernelGGL((fm_sdp_dups<GT, I64>), gw, dim3(256), 0, st, s, B);
}

// coalesce: this rank's lookups of n replicated tables -> (count, ids, g) payloads
extern "C" void fm_sdp_coalesce(int n, const void* const* idx, const int* idx64, const void* const* dy, const long* ldg,
                                const long* lo, const int* rows, const int* D, const int* bag, const float* scale,
                                int dy_bf16, long B, int* const* slot, int* const* cid, int* const* ids, float* const* g,
                                int* const* count, hipStream_t st) {
  if (B <= 0) return;
  for_each_width_batch(n, idx64, every_table, [&](const int* ks, int m, bool wide) {
    SdpSet s;
    int maxbag = 1;
    for (int i = 0; i < m; ++i) {
      const int k = ks[i];
      s.t[i] = SdpDesc{idx[k], dy[k], ldg[k], lo ? lo[k] : 0, rows[k], D[k], bag[k], scale[k], slot[k], cid[k], ids[k],
                       g[k], count[k]};
      maxbag = std::max(maxbag, bag[k]);
    }
    s.n = m;
    const long ne = B * maxbag;
    dim3 gc((unsigned)std::max<long>(1, std::min<long>((ne + 255) / 256, 1024)), m);
    dim3 gw((unsigned)std::max<long>(1, std::min<long>((ne + 3) / 4, 2048)), m);
    with_types(dy_bf16 != 0, wide, [&](auto t) {
      launch_coalesce<typename decltype(t)::elem, decltype(t)::wide>(s, gc, gw, B, st);
    });
  });
}

// apply the gathered segments in order: segs x n tables; seg_ids/seg_g/seg_count[s*n + k]; the
// own segment (own_seg) frees slot[k] and zeroes own_count[k] afterwards
extern "C" void fm_sdp_apply_segments(int n, int segs, int own_seg, float* const* W, const int* D, const int* const* seg_ids,
                                      const float* const* seg_g, const int* const* seg_count, int* const* slot,
                                      int* const* own_count, const int* nmax, const float* lr, hipStream_t st) {
  for_each_batch(n, every_table, [&](const int* ks, int m) {
    int nm = 1;
    for (int i = 0; i < m; ++i) nm = std::max(nm, nmax[ks[i]]);
    dim3 grid((unsigned)std::max(1, std::min((nm + 3) / 4, 2048)), m);
    CountSet zero;     // stays null (nothing zeroed) when own_seg is none of the segments
    for (int sg = 0; sg < segs; ++sg) {
      SdpApplySet s;
      for (int i = 0; i < m; ++i) {
        const int k = ks[i];
        const bool own = sg == own_seg;
        s.t[i] = SdpApply{W[k], seg_ids[sg * n + k], seg_g[sg * n + k], seg_count[sg * n + k], D[k], own ? slot[k] : nullptr,
                          own ? own_count[k] : nullptr};
        if (own) zero.c[i] = own_count[k];
      }
      s.n = m;
      hipLaunchKernelGGL(fm_sdp_apply, grid, dim3(256), 0, st, s, lr, nm);
    }
    if (own_seg >= 0 && own_seg < segs) hipLaunchKernelGGL(fm_emb_zero_counts, dim3(1), dim3(64), 0, st, zero);
  });
}

// ---- Adagrad apply launchers ------------------------------------------------------------------
// one payload (ids, g, count) per table from fm_sdp_coalesce (or the row-wise merge) -> H / W row
// updates, slots freed, counts zeroed; nmax[k] = capacity of table k's payload.  h_vec: H is read
// with 16-B accesses too and takes part in the alignment test (element-wise: H has the table's
// shape; row-wise: one fp32 per row, read as a scalar).
static void launch_adagrad_apply(void (*kernel)(AdaSet, const float*, float), bool h_vec, int n, float* const* W,
                                 float* const* H, const int* D, const int* const* ids, const float* const* g,
                                 int* const* count, int* const* slot, const int* nmax, const float* lr, float eps,
                                 hipStream_t st) {
  for_each_batch(n, every_table, [&](const int* ks, int m) {
    AdaSet s;
    CountSet zero;
    int nm = 1;
    for (int i = 0; i < m; ++i) {
      const int k = ks[i];
      const uintptr_t a = ((uintptr_t)W[k]) | ((uintptr_t)g[k]) | (h_vec ? (uintptr_t)H[k] : 0);
      const bool vec = D[k] % 4 == 0 && (a & 15) == 0;
      s.t[i] = AdaDesc{W[k], H[k], ids[k], g[k], count[k], slot[k], D[k], nmax[k], vec ? 1 : 0};
      zero.c[i] = count[k];
      nm = std::max(nm, nmax[k]);
    }
    s.n = m;
    // >= 4 rows per block-iteration in either form (element-wise: two in flight per lane in the vector form)
    dim3 grid((unsigned)std::max(1, std::min((nm + 7) / 8, 2048)), m);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, s, lr, eps);
    hipLaunchKernelGGL(fm_emb_zero_counts, dim3(1), dim3(64), 0, st, zero);
  });
}

extern "C" void fm_emb_adagrad_apply(int n, float* const* W, float* const* H, const int* D, const int* const* ids,
                                     const float* const* g, int* const* count, int* const* slot, const int* nmax,
                                     const float* lr, float eps, hipStream_t st) {
  launch_adagrad_apply(fm_emb_adagrad_apply_multi, true, n, W, H, D, ids, g, count, slot, nmax, lr, eps, st);
}

// h[k] holds one fp32 per table row
extern "C" void fm_emb_rowwise_adagrad_apply(int n, float* const* W, float* const* h, const int* D,
                                             const int* const* ids, const float* const* g, int* const* count,
                                             int* const* slot, const int* nmax, const float* lr, float eps,
                                             hipStream_t st) {
  launch_adagrad_apply(fm_emb_rowwise_apply_multi, false, n, W, h, D, ids, g, count, slot, nmax, lr, eps, st);
}

// release the own claims, then merge the segs gathered segments (seg_*[sg * n + k]) of n replicated
// tables in segment order into (mids, mg, mcount); mcount must be 0 on entry (the apply zeroes it)
extern "C" void fm_sdp_rowwise_merge_segments(int n, int segs, const int* rows, const int* D, const int* const* seg_ids,
                                              const float* const* seg_g, const int* const* seg_count,
                                              const int* const* own_ids, int* const* own_count, int* const* slot,
                                              int* const* mids, float* const* mg, int* const* mcount, const int* nmax,
                                              const int* mcap, hipStream_t st) {
  for_each_batch(n, every_table, [&](const int* ks, int m) {
    int nm = 1;
    RwReleaseSet rs;
    CountSet zero;
    for (int i = 0; i < m; ++i) {
      const int k = ks[i];
      rs.t[i] = RwRelease{own_ids[k], own_count[k], slot[k], rows[k], nmax[k]};
      zero.c[i] = own_count[k];
      nm = std::max(nm, nmax[k]);
    }
    rs.n = m;
    hipLaunchKernelGGL(fm_sdp_rowwise_release, dim3((unsigned)std::max(1, std::min((nm + 255) / 256, 1024)), m), dim3(256),
                       0, st, rs);
    hipLaunchKernelGGL(fm_emb_zero_counts, dim3(1), dim3(64), 0, st, zero);
    dim3 grid((unsigned)std::max(1, std::min((nm + 3) / 4, 2048)), m);
    for (int sg = 0; sg < segs; ++sg) {
      RwMergeSet s;
      for (int i = 0; i < m; ++i) {
        const int k = ks[i];
        const float* gs = seg_g[sg * n + k];
        const bool vec = D[k] % 4 == 0 && ((((uintptr_t)gs) | ((uintptr_t)mg[k])) & 15) == 0;
        s.t[i] = RwMerge{seg_ids[sg * n + k], gs, seg_count[sg * n + k], slot[k], mids[k], mg[k], mcount[k],
                         rows[k], D[k], nmax[k], mcap[k], vec ? 1 : 0};
      }
      s.n = m;
      hipLaunchKernelGGL(fm_sdp_rowwise_merge, grid, dim3(256), 0, st, s);
    }
  });
}
