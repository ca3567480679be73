// GELU (exact erf form), tanh-GELU and SiLU with their derivatives, as functions of the PRE-activation z:
// none of them is monotonic, so the derivative cannot be expressed through the output.  The codes are the
// unary codes of flexmi/ops/elementwise.py; elementwise.hip (fm_unary_*) and act_gemm.hip share this file.
//
// All three are z * gate(z) with a gate in (0, 1), written so that the gate keeps its relative precision in the
// negative tail, where y = z * gate is small: Phi(z) = erfc(-z / sqrt 2) / 2 (not (1 + erf) / 2, which cancels),
// and (1 + tanh u) / 2 = sigmoid(2 u) exactly.
#pragma once
#include "common.h"

enum { ACTZ_GELU = 5, ACTZ_GELU_TANH = 6, ACTZ_SILU = 7 };

FM_HOST_DEVICE bool actz_known(int code) { return code >= ACTZ_GELU && code <= ACTZ_SILU; }

FM_DEVICE float actz_sigmoid(float z) { return 1.f / (1.f + __expf(-z)); }
FM_DEVICE float actz_cdf(float z) { return 0.5f * erfcf(z * -0.70710678118654752f); }
// 2 u(z) = 2 sqrt(2 / pi) (z + 0.044715 z^3) and its derivative
FM_DEVICE float actz_2u(float z) { return 1.5957691216057308f * z * fmaf(0.044715f, z * z, 1.f); }
FM_DEVICE float actz_d2u(float z) { return 1.5957691216057308f * fmaf(0.134145f, z * z, 1.f); }

FM_DEVICE float actz_fwd(int code, float z) {
  if (code == ACTZ_SILU) return z * actz_sigmoid(z);
  if (code == ACTZ_GELU) return z * actz_cdf(z);
  return z * actz_sigmoid(actz_2u(z));
}

// silu' = s (1 + z (1 - s));  gelu' = Phi + z phi;  tanh form with s = sigmoid(2 u): s + z s (1 - s) (2 u)'
FM_DEVICE float actz_dfwd(int code, float z) {
  if (code == ACTZ_GELU) return actz_cdf(z) + z * 0.39894228040143268f * __expf(-0.5f * z * z);
  const bool silu = code == ACTZ_SILU;
  const float s = actz_sigmoid(silu ? z : actz_2u(z));
  return s * (1.f + z * (1.f - s) * (silu ? 1.f : actz_d2u(z)));
}
