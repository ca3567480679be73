"""OCP MX (microscaling) fp8 tensors: the format, and its reference arithmetic in plain torch.

An MX tensor is fp8 codes plus one E8M0 scale byte per block of 32 consecutive elements along the
contraction dimension (OCP MX v1.0): ``value = code * 2^(byte - 127)``.  For a block with largest
magnitude ``amax``:

    e    = clamp(floor(log2 amax) - emax, -127, 127)     emax = 8 (e4m3, max 448) / 15 (e5m2, max 57344)
    byte = e + 127
    code = RNE_fp8(clamp(v * 2^-e, -max, +max))

The clamp is explicit and done in fp32: the block's top value can reach 1.99 * 2^emax, and neither
torch's float8 casts nor the gfx950 conversion instructions saturate (they give NaN / inf).  ``floor(log2
amax)`` is read from amax's fp32 exponent field, so a zero block (and an fp32-subnormal one) gets ``e =
-127``, scale byte 0 and zero codes.  NaN and inf inputs are out of scope: nothing here or in
``csrc/kernels/mxfp8.hip`` looks for them.

:func:`mx_quantize_torch` is the CPU backend's arithmetic and the oracle of the GPU tests: the HIP
quantisers give the same codes and scale bytes bit for bit.
"""
from __future__ import annotations

import torch

BLOCK = 32
FMT_E4M3, FMT_E5M2 = 0, 1          # the kernels' format codes (also the instruction's cbsz / blgp)
_DTYPE = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
_EMAX = {"e4m3": 8, "e5m2": 15}
_MAX = {"e4m3": 448.0, "e5m2": 57344.0}
FMT_CODE = {"e4m3": FMT_E4M3, "e5m2": FMT_E5M2}


def pad128(n):
    """Rows of a column-wise copy: ``n`` rounded up to a multiple of 128 (the GEMM's k step)."""
    return (n + 127) // 128 * 128


def mx_quantize_torch(t, dim, fmt):
    """Quantise ``t`` (any float dtype, computed in fp32) in blocks of 32 along ``dim``, whose size must be
    a multiple of 32.  Returns ``(codes, scales, deq)``: codes as a ``torch.float8_*`` tensor of ``t``'s
    shape, scale bytes (uint8) with ``dim`` shrunk by 32, and the dequantised fp32 tensor ``code *
    2^(byte - 127)``, which is exact.  NaN / inf inputs are out of scope."""
    x = t.detach().float().movedim(dim, -1)
    shape = x.shape
    assert shape[-1] % BLOCK == 0, f"mx_quantize_torch: {shape[-1]} elements along dim {dim} are not a multiple of 32"
    xb = x.reshape(*shape[:-1], shape[-1] // BLOCK, BLOCK)
    amax = xb.abs().amax(-1, keepdim=True).contiguous()
    e = ((amax.view(torch.int32) >> 23) & 0xFF) - 127 - _EMAX[fmt]
    e = e.clamp(-127, 127)
    scaled = torch.ldexp(xb, -e).clamp(-_MAX[fmt], _MAX[fmt])
    codes = scaled.to(_DTYPE[fmt])
    deq = torch.ldexp(codes.float(), e)
    back = lambda v: v.reshape(shape).movedim(-1, dim).contiguous()  # noqa: E731
    scales = (e + 127).to(torch.uint8).squeeze(-1).movedim(-1, dim).contiguous()
    return back(codes.view(torch.uint8)).view(_DTYPE[fmt]), scales, back(deq)
