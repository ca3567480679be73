// The dense update rules (SGD, Adagrad, Adam) and the one traversal that applies a rule to a range
// of a rank's flat fp32 buffers.  This is the only place in csrc/kernels/ where a rule's
// arithmetic is written: the optimizer launches (optim.hip), the fused dW-SGD GEMM epilogues
// (gemm_epilogue.h sgd_apply1 / sgd_apply4) and the small-K reduce (gemm_small.hip) all call it, so
// scalar head, 16-B body, scalar tail and every fused form compute the same values.
#pragma once
#include "common.h"

namespace {

// lane-wise sqrt and a * b + c in one rounding, for the two lane types the rules run on: one
// element, or four at a 16-B boundary
FM_DEVICE float lane_sqrt(float x) { return sqrtf(x); }
FM_DEVICE f32x4_t lane_sqrt(f32x4_t x) { return f32x4_t{sqrtf(x[0]), sqrtf(x[1]), sqrtf(x[2]), sqrtf(x[3])}; }
FM_DEVICE float lane_fma(float a, float b, float c) { return fmaf(a, b, c); }
FM_DEVICE f32x4_t lane_fma(f32x4_t a, f32x4_t b, f32x4_t c) {
  return f32x4_t{fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1]), fmaf(a[2], b[2], c[2]), fmaf(a[3], b[3], c[3])};
}

// A rule: NS state arrays and operator()(w, g, step, s): the new w from w, the gradient g, the
// device-side step size (lr, or Adam's bias-corrected alpha_t) and pointers s to its state values,
// which it advances in place -- in memory, so a rule that keeps no state under its constants (SGD
// without momentum) never touches it and the pointer may be null.  Written once, lane-wise, for
// T = float and T = f32x4_t.

// g = G + wd W; V = mom V + g; g = nesterov ? g + mom V : V (only if mom > 0); W -= lr g
struct SgdRule {
  static constexpr int NS = 1;
  float wd, mom;
  int nesterov;
  template <class T>
  FM_DEVICE T operator()(T w, T g, float lr, T* const (&s)[1]) const {
    g += wd * w;
    if (mom > 0.f) {
      const T v = *s[0] * mom + g;
      *s[0] = v;
      g = nesterov ? g + mom * v : v;
    }
    return w - lr * g;
  }
};

// torch.optim.Adagrad with lr_decay = 0: g = G + wd W; H += g g; W -= lr g / (sqrt(H) + eps)
struct AdagradRule {
  static constexpr int NS = 1;
  float wd, eps;
  template <class T>
  FM_DEVICE T operator()(T w, T g, float lr, T* const (&s)[1]) const {
    g += wd * w;
    const T h = *s[0] + g * g;
    *s[0] = h;
    return w - lr * g / (lane_sqrt(h) + eps);
  }
};

// g = G + wd W; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; W -= alpha_t m / (sqrt(v) + eps)
struct AdamRule {
  static constexpr int NS = 2;
  float b1, b2, wd, eps;
  template <class T>
  FM_DEVICE T operator()(T w, T g, float alpha_t, T* const (&s)[2]) const {
    g += wd * w;
    // the fused multiply-adds spelled out: which product of a sum of two the compiler fuses is its
    // choice, and it is not the same choice in every context
    const T m = lane_fma(T(1.f - b1), g, b1 * *s[0]);
    const T v = lane_fma((1.f - b2) * g, g, b2 * *s[1]);
    *s[0] = m;
    *s[1] = v;
    return w - alpha_t * m / (lane_sqrt(v) + eps);
  }
};

// The buffers a rule runs over: fp32 master W, its state arrays S and the bf16 mirror Wc (or null)
template <class R>
struct UpdBufs {
  float* W;
  float* S[R::NS];
  unsigned short* Wc;
};

// the bf16 mirror of one element / the packed mirror of four
FM_DEVICE void store_mirror(unsigned short* p, float w) { *p = f2bf(w); }
FM_DEVICE void store_mirror(unsigned short* p, const f32x4_t& w) {
  bf16x4_t c;
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = (short)f2bf(w[j]);
  *reinterpret_cast<bf16x4_t*>(p) = c;
}

// The rule at offset e with gradient g.  T = float: one element.  T = f32x4_t: four lanes at an
// offset where W and S are 16-B aligned (Wc 8-B) -- b128 loads, the rule per lane, b128 stores and
// the packed mirror store.
template <class R, class T>
FM_DEVICE void update_lanes(const R& r, const UpdBufs<R>& b, float step, long e, T g) {
  T* s[R::NS];
#pragma unroll
  for (int k = 0; k < R::NS; ++k) s[k] = reinterpret_cast<T*>(b.S[k] + e);
  const T w = r(*reinterpret_cast<const T*>(b.W + e), g, step, s);
  *reinterpret_cast<T*>(b.W + e) = w;
  if (b.Wc) store_mirror(b.Wc + e, w);
}

// The rule over [o, o + n) of the flat buffers, by the blocks of grid dimension x: scalar head up
// to the 16-B boundary, vector body, scalar tail.  h0 = update_head() of the buffers' bases
// (< 0: every element scalar).  zero_g: the gradient is consumed here -- it is written back as 0
// so the next backward starts from a clean accumulator without a separate memset.
template <class R>
FM_DEVICE void update_range(const R& r, const UpdBufs<R>& b, float* __restrict__ G, float step, long o, long n, int h0,
                            int zero_g) {
  const long head = h0 < 0 ? 0 : min(n, (long)((h0 - o) & 3));
  const long n4 = h0 < 0 ? 0 : (n - head) / 4;
  const long stride = (long)gridDim.x * blockDim.x, t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  auto one = [&](long i) {
    const float g = G[i];
    if (zero_g) G[i] = 0.f;
    update_lanes(r, b, step, i, g);
  };
  for (long i = t0; i < head; i += stride) one(o + i);
  for (long i = t0; i < n4; i += stride) {
    const long e = o + head + 4 * i;
    const f32x4_t g = *reinterpret_cast<const f32x4_t*>(G + e);
    if (zero_g) *reinterpret_cast<f32x4_t*>(G + e) = f32x4_t{0.f, 0.f, 0.f, 0.f};
    update_lanes(r, b, step, e, g);
  }
  for (long i = head + 4 * n4 + t0; i < n; i += stride) one(o + i);
}

}  // namespace

// Elements of the buffers' bases before their first common 16-B boundary (8-B for the bf16 mirror
// Wc), 0..3; -1 when W, G, the ns state arrays S (null entries skipped) and Wc are not congruent
// modulo their vector width, and the whole range has to go scalar.
static inline int update_head(const float* W, const float* G, float* const* S, int ns, const unsigned short* Wc) {
  const uintptr_t a = (uintptr_t)W & 15;
  bool ok = (a & 3) == 0 && ((uintptr_t)G & 15) == a;
  for (int k = 0; k < ns; ++k) ok = ok && (!S[k] || ((uintptr_t)S[k] & 15) == a);
  ok = ok && (!Wc || ((uintptr_t)Wc & 7) == a / 2);
  return ok ? (int)(((16 - a) & 15) / 4) : -1;
}
