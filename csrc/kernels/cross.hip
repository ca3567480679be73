// DCNv2 cross-layer combine (Wang et al. 2021, "DCN V2", eq. 2 with the low-rank U·V of eq. 5):
//   y = x0 ⊙ t + x          t = U (V x) + b comes from two ordinary Linear ops
// One streaming pass per direction, after elementwise.hip: 8 consecutive elements per
// thread-iteration (one 16-B access per bf16 operand, two per fp32 operand) when every operand is
// 16-B aligned, a scalar tail, and the scalar form for everything otherwise; grid capped by
// fm_grid with a grid-stride loop.  Arithmetic in fp32, bf16 rounded once on store.
//   forward : reads x0, t, x                     writes y
//   backward: reads dy, x0 (for dt), t (for dx0) writes dt = dy ⊙ x0, dx0 (+)= dy ⊙ t, dx (+)= dy
// x == nullptr is the first layer's form (x_l is x_0 itself): y = x0 ⊙ t + x0 and dx0 also takes
// dy, so no op ever receives one tensor as two inputs.  A null dt / dx0 / dx is skipped.
#include "common.h"

namespace {

template <typename T>
__global__ void fm_cross_fwd(const T* __restrict__ x0, const T* __restrict__ t, const T* __restrict__ x, T* __restrict__ y,
                             long n, int vec) {
  const long stride = (long)gridDim.x * blockDim.x;
  long i0 = 0;
  if (vec) {
    const long n8 = n / 8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += stride) {
      float a[8], b[8], c[8];
      ld8<T>(x0 + 8 * i, a);
      ld8<T>(t + 8 * i, b);
      if (x) ld8<T>(x + 8 * i, c);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = a[j] * b[j] + (x ? c[j] : a[j]);
      st8<T>(y + 8 * i, a);
    }
    i0 = n8 * 8;
  }
  for (long i = i0 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float a = ld<T>(x0 + i);
    st<T>(y + i, a * ld<T>(t + i) + (x ? ld<T>(x + i) : a));
  }
}

// self: the two-input form (dx0 also takes dy; dx is null then)
template <typename T>
__global__ void fm_cross_bwd(const T* __restrict__ dy, const T* __restrict__ x0, const T* __restrict__ t, T* __restrict__ dt,
                             T* __restrict__ dx0, T* __restrict__ dx, long n, int acct, int acc0, int accx, int self,
                             int vec) {
  const long stride = (long)gridDim.x * blockDim.x;
  long i0 = 0;
  if (vec) {
    const long n8 = n / 8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += stride) {
      float g[8], o[8], r[8];
      ld8<T>(dy + 8 * i, g);
      if (dt) {
        ld8<T>(x0 + 8 * i, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = g[j] * o[j];
        if (acct) {
          ld8<T>(dt + 8 * i, o);
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] += o[j];
        }
        st8<T>(dt + 8 * i, r);
      }
      if (dx0) {
        ld8<T>(t + 8 * i, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = g[j] * o[j] + (self ? g[j] : 0.f);
        if (acc0) {
          ld8<T>(dx0 + 8 * i, o);
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] += o[j];
        }
        st8<T>(dx0 + 8 * i, r);
      }
      if (dx) {
        if (accx) {
          ld8<T>(dx + 8 * i, o);
#pragma unroll
          for (int j = 0; j < 8; ++j) g[j] += o[j];
        }
        st8<T>(dx + 8 * i, g);
      }
    }
    i0 = n8 * 8;
  }
  for (long i = i0 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
    const float g = ld<T>(dy + i);
    if (dt) st<T>(dt + i, g * ld<T>(x0 + i) + (acct ? ld<T>(dt + i) : 0.f));
    if (dx0) st<T>(dx0 + i, g * ld<T>(t + i) + (self ? g : 0.f) + (acc0 ? ld<T>(dx0 + i) : 0.f));
    if (dx) st<T>(dx + i, g + (accx ? ld<T>(dx + i) : 0.f));
  }
}

bool al16(const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" void fm_cross_forward(const void* x0, const void* t, const void* x, void* y, long n, int bf16, hipStream_t s) {
  if (n <= 0) return;
  const int vec = al16(x0) && al16(t) && al16(x) && al16(y);
  const dim3 grid(fm_grid((n + 7) / 8));
  if (bf16)
    hipLaunchKernelGGL((fm_cross_fwd<unsigned short>), grid, dim3(256), 0, s, (const unsigned short*)x0, (const unsigned short*)t,
                       (const unsigned short*)x, (unsigned short*)y, n, vec);
  else
    hipLaunchKernelGGL((fm_cross_fwd<float>), grid, dim3(256), 0, s, (const float*)x0, (const float*)t, (const float*)x,
                       (float*)y, n, vec);
}

extern "C" void fm_cross_backward(const void* dy, const void* x0, const void* t, void* dt, void* dx0, void* dx, long n, int acct,
                                  int acc0, int accx, int self, int bf16, hipStream_t s) {
  if (n <= 0 || (!dt && !dx0 && !dx)) return;
  const int vec = al16(dy) && al16(x0) && al16(t) && al16(dt) && al16(dx0) && al16(dx);
  const dim3 grid(fm_grid((n + 7) / 8));
  if (bf16)
    hipLaunchKernelGGL((fm_cross_bwd<unsigned short>), grid, dim3(256), 0, s, (const unsigned short*)dy, (const unsigned short*)x0,
                       (const unsigned short*)t, (unsigned short*)dt, (unsigned short*)dx0, (unsigned short*)dx, n, acct, acc0,
                       accx, self, vec);
  else
    hipLaunchKernelGGL((fm_cross_bwd<float>), grid, dim3(256), 0, s, (const float*)dy, (const float*)x0, (const float*)t,
                       (float*)dt, (float*)dx0, (float*)dx, n, acct, acc0, accx, self, vec);
}
