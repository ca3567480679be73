// Streaming ROC AUC: per-class score histogram (flexmi/core/loss_metrics.py, METRICS_AUC).
//
// A score s (fp32, or bf16 widened exactly) is keyed by the monotone total order over floats
//   u = bits(s);  -0.0 -> +0.0;  u = (u >> 31) ? ~u : (u | 0x80000000);  bin = u >> shift
// and counted in hist[label >= 0.5][bin] (int64, [2][1 << (32 - shift)]); NaN scores are counted in
// *invalid and nowhere else.  Integer counts: the result does not depend on arrival order.
//
// Contention: a model whose scores sit in a handful of bins (all equal is the extreme) makes one
// 64-bit atomic per sample serialise on a few lines: 75 us at B = 8192, 590 us at 65536, against
// 3-5 us for distinct scores (profiles/auc_hist_ab.txt).  Each wave therefore combines equal
// (class, bin) keys before the atomic with a peel loop over its live lanes: broadcast the first live
// lane's key, ballot the lanes that hold it, that lane adds the popcount once, the matched lanes
// retire.  A full peel costs a wave of distinct scores 64 rounds (10 us against 3.5 us), so the
// loop gives up once `rounds` of its rounds have found a key that no other lane shares, and the
// lanes still live add 1 each: heavy keys are the likeliest to sit on the first live lane, and what
// is left after a few lone keys is spread over many bins, where plain atomics do not contend.
// rounds = 0 is one atomic per sample, 64 the full peel (tools/bench_auc.py times all three).  The
// batch loop is block-uniform, so every lane of a wave reaches every ballot; lanes past B and NaN
// lanes are never live.
#include "common.h"

#define FM_AUC_PEEL_ROUNDS 2

namespace {

template <typename ST>
__global__ void __launch_bounds__(256) fm_auc_hist_kernel(const ST* __restrict__ scores, const float* __restrict__ labels,
                                                         long B, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ invalid, int shift, int rounds) {
  const int lane = threadIdx.x & 63;
  const int cls_shift = 32 - shift;      // slot = class << cls_shift | bin  (< 2^(33 - shift), shift >= 1)
  const long stride = (long)gridDim.x * blockDim.x;
  for (long b0 = blockIdx.x * (long)blockDim.x; b0 < B; b0 += stride) {
    const long b = b0 + threadIdx.x;
    bool live = b < B, nan = false;
    unsigned slot = 0;
    if (live) {
      unsigned u = __float_as_uint(ld<ST>(scores + b));
      if (u == 0x80000000u) u = 0u;                       // s + 0.0f: -0.0 and +0.0 compare equal
      nan = (u & 0x7fffffffu) > 0x7f800000u;
      u = (u >> 31) ? ~u : (u | 0x80000000u);
      slot = ((labels[b] >= 0.5f ? 1u : 0u) << cls_shift) | (u >> shift);
      live = !nan;
    }
    const unsigned long long bad = __ballot(nan);
    if (bad && lane == (int)__ffsll((long long)bad) - 1) atomicAdd(invalid, (unsigned long long)__popcll(bad));
    unsigned long long todo = __ballot(live);
    int lone = 0;                                         // rounds that folded nothing
    while (todo && lone < rounds) {                       // wave-uniform: todo and same come from ballots
      const int leader = (int)__ffsll((long long)todo) - 1;
      const unsigned key = (unsigned)__shfl((int)slot, leader, 64);
      const unsigned long long same = __ballot(live && slot == key);
      if (lane == leader) atomicAdd(hist + key, (unsigned long long)__popcll(same));
      live = live && slot != key;
      todo &= ~same;
      lone += (same & (same - 1)) == 0;
    }
    if (live) atomicAdd(hist + slot, 1ull);
  }
}

}  // namespace

// rounds: lone-key peel rounds a wave tolerates before its remaining lanes add 1 each (0 .. 64; < 0: the default)
extern "C" void fm_auc_hist_variant(const void* scores, int scores_bf16, const float* labels, long B, long long* hist,
                                    long long* invalid, int shift, int rounds, hipStream_t s) {
  if (B <= 0 || shift < 1 || shift > 31) return;
  rounds = rounds < 0 ? FM_AUC_PEEL_ROUNDS : std::min(rounds, 64);
  dim3 g(fm_grid(B, 256, 1024));
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  unsigned long long* iv = reinterpret_cast<unsigned long long*>(invalid);
  if (scores_bf16)
    hipLaunchKernelGGL(fm_auc_hist_kernel<unsigned short>, g, dim3(256), 0, s, (const unsigned short*)scores, labels, B, h, iv,
                       shift, rounds);
  else
    hipLaunchKernelGGL(fm_auc_hist_kernel<float>, g, dim3(256), 0, s, (const float*)scores, labels, B, h, iv, shift, rounds);
}
