// Fused optimizer updates over a rank's flat parameter buffer (replaces the per-parameter Legion
// tasks of src/runtime/optimizer_kernel.cu:23-41 sgd_update and :134-154 adam_update, and the
// gradient-replica sums of :96-101 / :220-225 which RCCL all-reduce now does).
// ONE launch updates every parameter shard of the rank: fp32 master weights, optional momentum /
// Adam / Adagrad state, and the bf16 compute mirror written in the same pass (no separate cast kernel).
// Vectorised 16-B loads/stores; lr is read from device memory so the step is graph-capturable.
#include "update_rule.h"

namespace {

// One rule over one flat range: a thin launch of update_rule.h's traversal
template <class R>
__global__ void fm_update_kernel(R r, UpdBufs<R> b, float* __restrict__ G, const float* __restrict__ step_p, long n, int h0,
                                 int zero_g) {
  update_range(r, b, G, step_p[0], 0, n, h0, zero_g);
}

// The same over up to 32 disjoint ranges of one flat buffer (blockIdx.y = range): the parameters
// left to the optimizer launch when most weights were updated inside their dW GEMMs (gemm.hip
// fm_gemm_dw_sgd) -- one launch instead of one per bias-sized gap.
struct UpdSegs {
  long off[32];
  long len[32];
};

template <class R>
__global__ void fm_update_segs_kernel(R r, UpdBufs<R> b, float* __restrict__ G, const float* __restrict__ step_p,
                                      UpdSegs segs, int h0, int zero_g) {
  update_range(r, b, G, step_p[0], segs.off[blockIdx.y], segs.len[blockIdx.y], h0, zero_g);
}

// grid of the flat forms: one 4-element group per thread on the vector path
template <class R>
void update_flat(const R& r, const UpdBufs<R>& b, float* G, const float* step, long n, int zero_g, hipStream_t s) {
  if (n <= 0) return;
  const int h0 = update_head(b.W, G, b.S, R::NS, b.Wc);
  hipLaunchKernelGGL(fm_update_kernel<R>, dim3(fm_grid(h0 < 0 ? n : n / 4 + 1)), dim3(256), 0, s, r, b, G, step, n, h0,
                     zero_g);
}

__global__ void fm_cast_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = f2bf(src[i]);
}

}  // namespace

extern "C" void fm_sgd_update(float* W, float* G, float* V, unsigned short* Wc, const float* lr, long n, float wd,
                              float mom, int nesterov, int zero_g, hipStream_t s) {
  update_flat(SgdRule{wd, mom, nesterov}, UpdBufs<SgdRule>{W, {mom > 0.f ? V : nullptr}, Wc}, G, lr, n, zero_g, s);
}

extern "C" void fm_sgd_update_segs(float* W, float* G, float* V, unsigned short* Wc, const float* lr, const long* off,
                                   const long* len, int nseg, float wd, float mom, int nesterov, int zero_g,
                                   hipStream_t s) {
  const SgdRule r{wd, mom, nesterov};
  const UpdBufs<SgdRule> bufs{W, {mom > 0.f ? V : nullptr}, Wc};
  const int h0 = update_head(W, G, bufs.S, 1, Wc);
  for (int b = 0; b < nseg; b += 32) {
    UpdSegs sg;
    long mx = 0;
    const int k = nseg - b < 32 ? nseg - b : 32;
    for (int i = 0; i < 32; ++i) {
      sg.off[i] = i < k ? off[b + i] : 0;
      sg.len[i] = i < k ? len[b + i] : 0;
      mx = sg.len[i] > mx ? sg.len[i] : mx;
    }
    if (mx <= 0) continue;
    const long per = (mx + 3) / 4;   // one 4-element group per thread
    const int gx = (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024);
    hipLaunchKernelGGL(fm_update_segs_kernel<SgdRule>, dim3(gx, k), dim3(256), 0, s, r, bufs, G, lr, sg, h0, zero_g);
  }
}

extern "C" void fm_adam_update(float* W, float* G, float* M, float* V, unsigned short* Wc, long n,
                               const float* alpha_t, float b1, float b2, float wd, float eps, int zero_g,
                               hipStream_t s) {
  update_flat(AdamRule{b1, b2, wd, eps}, UpdBufs<AdamRule>{W, {M, V}, Wc}, G, alpha_t, n, zero_g, s);
}

extern "C" void fm_adagrad_update(float* W, float* G, float* H, unsigned short* Wc, const float* lr, long n, float wd,
                                  float eps, int zero_g, hipStream_t s) {
  update_flat(AdagradRule{wd, eps}, UpdBufs<AdagradRule>{W, {H}, Wc}, G, lr, n, zero_g, s);
}

extern "C" void fm_cast_bf16(const float* src, unsigned short* dst, long n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fm_cast_bf16_kernel, dim3(fm_grid(n)), dim3(256), 0, s, src, dst, n);
}
