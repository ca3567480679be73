"""Pooling and batch norm (csrc/kernels/cnn.hip) on every dispatch path, against fp64 torch oracles.

Pooling: planes of more than one row band (windows whose maximum lies in the neighbouring band, the
plo / phi staging arithmetic), several planes per block, the per-output forward past the band
kernels' LDS limit, the max scatter at one input row per band and the row-segment backward; windows,
strides and pads that differ between h and w, a fused ReLU, and ties under PyTorch's first-maximum
rule from both argmax sources.  Every case asserts through ``pool_last_form()`` that it ran the kernel
it is here for, so a later re-dispatch cannot empty it.

Batch norm: more elements per channel than the statistics grid covers in one pass, accumulation
into dx, dx=None, the saved statistics, and inputs far from zero (mean / std = 100), where a one-pass
variance E[x^2] - mean^2 loses its digits."""
import pytest
import torch
import torch.nn.functional as F

from flexmi.ops import _kernels as Kk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MAX, AVG = 30, 31
NONE, RELU = 10, 11

#        H   W    kh kw sh sw pt pl   forward form        max backward        avg backward
ROWS = {
    "two_bands": ((40, 130, 3, 3, 2, 2, 1, 1), ("band", 2, 1), ("scatter", 2, 1), ("band", 2, 1)),
    "two_bands_asym": ((70, 70, 3, 2, 2, 1, 1, 0), ("band", 2, 1), ("scatter", 2, 1), ("band", 2, 1)),
    "six_planes_asym": ((23, 19, 5, 2, 3, 1, 2, 0), ("planes", 1, 6), ("scatter", 1, 6), ("band", 1, 6)),
    # kh * W > 4096: per-output forward; one input row per scatter band; the avg gather would stage
    # 4 x 2500 windows x 5 B = 50000 B > 48 KiB: row segments.  W % 8 = 4, bf16 rows 5000 B apart
    "wide": ((4, 2500, 3, 3, 1, 1, 1, 1), ("per_output", 0, 0), ("scatter", 4, 1), ("rows", 0, 0)),
    # the same three kernels with h and w apart (4 x 2499 windows x 5 B = 49980 B)
    "wide_asym": ((8, 2500, 5, 2, 2, 1, 2, 0), ("per_output", 0, 0), ("scatter", 8, 1), ("rows", 0, 0)),
}
N_, C_ = 2, 3


def _ref_pool(xd, geo, is_max, act):
    H, W, kh, kw, sh, sw, pt, pl = geo
    if is_max:
        r = F.max_pool2d(xd, (kh, kw), (sh, sw), (pt, pl))
    else:
        r = F.avg_pool2d(xd, (kh, kw), (sh, sw), (pt, pl), count_include_pad=False)
    return torch.relu(r) if act == RELU else r


def _forms():
    f = Kk.pool_last_form()
    return tuple(f["fwd"]), tuple(f["bwd"])


def _run_pool(gpu, x, dy, geo, is_max, act, forms, tol, exact=False):
    """Forward, then the backward with acc off / on and (max) the argmax bytes from the forward /
    recomputed by the backward, each against autograd of the fp64 reference on the same values."""
    H, W, kh, kw, sh, sw, pt, pl = geo
    fwd_form, max_form, avg_form = forms
    kind = MAX if is_max else AVG
    xr = x.double().requires_grad_(True)
    ref = _ref_pool(xr, geo, is_max, act)
    gx, = torch.autograd.grad(ref, [xr], dy.double())
    ref = ref.detach()
    y = torch.full(ref.shape, -7.0, device=gpu, dtype=x.dtype)
    saved = {}
    Kk.pool2d_forward(x, y, (kh, kw), (sh, sw), (pt, pt, pl, pl), kind, act, saved)
    assert _forms()[0] == fwd_form
    if exact:
        assert torch.equal(y.double(), ref)
    else:
        torch.testing.assert_close(y.double(), ref, rtol=tol, atol=tol)
    for recorded in ((True, False) if is_max else (True,)):
        for acc in (False, True):
            base = torch.randint(-3, 4, x.shape, device=gpu).to(x.dtype) if acc else torch.full_like(x, -7.0)
            dx = base.clone()
            Kk.pool2d_backward(x, y, dy, dx, (kh, kw), (sh, sw), (pt, pt, pl, pl), kind, act, acc,
                               saved if recorded else {})
            assert _forms()[1] == (max_form if is_max else avg_form)
            exp = gx + (base.double() if acc else 0)
            if exact:
                assert torch.equal(dx.double(), exp), (recorded, acc)
            else:
                torch.testing.assert_close(dx.double(), exp, rtol=2 * tol, atol=2 * tol)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_pool_forms(gpu, dt, is_max, row):
    geo, *forms = ROWS[row]
    torch.manual_seed(geo[0] * geo[1])
    x = torch.randn(N_, C_, geo[0], geo[1], device=gpu).to(dt)
    P, Q = _ref_pool(x[:1, :1].double(), geo, is_max, NONE).shape[2:]
    dy = torch.randn(N_, C_, P, Q, device=gpu).to(dt)
    _run_pool(gpu, x, dy, geo, is_max, NONE, forms, 1e-6 if dt == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("row", ["two_bands", "six_planes_asym"])
def test_pool_fused_relu(gpu, dt, is_max, row):
    """act = ReLU: the forward is relu(pool), the backward masks dy by y > 0."""
    geo, *forms = ROWS[row]
    torch.manual_seed(geo[0] + geo[1])
    x = torch.randn(N_, C_, geo[0], geo[1], device=gpu).sub_(1.5 if is_max else 0.0).to(dt)
    P, Q = _ref_pool(x[:1, :1].double(), geo, is_max, NONE).shape[2:]
    dy = torch.randn(N_, C_, P, Q, device=gpu).to(dt)
    ref = _ref_pool(x.double(), geo, is_max, RELU)
    share = (ref > 0).double().mean().item()
    assert 0.2 < share < 0.8, share          # the mask must matter
    _run_pool(gpu, x, dy, geo, is_max, RELU, forms, 1e-6 if dt == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("row", ["two_bands", "six_planes_asym"])
def test_pool_max_ties_first_maximum(gpu, dt, row):
    """Inputs from {0, 1, 2} and integer gradients (exact in bf16): nearly every window ties, the
    gradient goes to the FIRST maximum in row-major order, as in PyTorch; everything is exact."""
    geo, *forms = ROWS[row]
    torch.manual_seed(geo[1])
    x = torch.randint(0, 3, (N_, C_, geo[0], geo[1]), device=gpu).to(dt)
    P, Q = _ref_pool(x[:1, :1].double(), geo, True, NONE).shape[2:]
    dy = torch.randint(-3, 4, (N_, C_, P, Q), device=gpu).to(dt)
    _run_pool(gpu, x, dy, geo, True, NONE, forms, 0.0, exact=True)


# ---------------------------------------------------------------- batch norm
TOL = 1e-4          # the fp32 bound of tests/test_gpu_fp32.py (max-normalised relative error)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 96, 96), (3, 5, 7, 9)])      # 18432 per channel > 64 x 256
def test_batchnorm_forms(gpu, dt, relu, shape):
    torch.manual_seed(shape[2])
    ty, tg, tx = (TOL, TOL, TOL) if dt == torch.float32 else (1e-2, 2e-2, 3e-2)
    x = (torch.randn(*shape, device=gpu) * 2 + 0.5).to(dt)
    Cn = shape[1]
    gamma, beta = torch.rand(Cn, device=gpu) + 0.5, torch.randn(Cn, device=gpu)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.batch_norm(xd, None, None, gd, bd, training=True, eps=1e-5)
    if relu:
        yr = torch.relu(yr)
    dy = torch.randn(*shape, device=gpu).to(dt)
    gx, gg, gb = torch.autograd.grad(yr, [xd, gd, bd], dy.double())
    y = torch.empty_like(x)
    saved = {}
    Kk.batchnorm_forward(x, gamma, beta, y, relu, 1e-5, saved)
    assert rel_err(y, yr.detach()) < ty
    mean = x.double().mean((0, 2, 3))
    inv = (x.double().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    assert rel_err(saved["bn_meaninv"][:Cn], mean) < TOL
    assert rel_err(saved["bn_meaninv"][Cn:], inv) < TOL
    for acc in (False, True):
        base = torch.randn(*shape, device=gpu).to(dt) if acc else torch.full_like(x, -7.0)
        dx = base.clone()
        dgam, dbet = torch.full((Cn,), -7.0, device=gpu), torch.full((Cn,), -7.0, device=gpu)
        Kk.batchnorm_backward(x, gamma, y, dy, dx, dgam, dbet, relu, 1e-5, saved, acc)
        assert rel_err(dx, gx + (base.double() if acc else 0)) < tx
        assert rel_err(dgam, gg) < tg
        assert rel_err(dbet, gb) < tg
    # dx=None: the parameter gradients alone
    dgam, dbet = torch.full((Cn,), -7.0, device=gpu), torch.full((Cn,), -7.0, device=gpu)
    Kk.batchnorm_backward(x, gamma, y, dy, None, dgam, dbet, relu, 1e-5, saved, False)
    assert rel_err(dgam, gg) < tg
    assert rel_err(dbet, gb) < tg


def test_batchnorm_offset_inputs(gpu):
    """fp32 inputs at mean / std = 100.  The bound is what torch's own fp32 batch norm (CPU) loses
    against fp64 on the same input, times 10 for the atomic summation order and rsqrtf; the one-pass
    E[x^2] - mean^2 variance without a pivot was 200x off that (6.4e-4 against 3.4e-6 in emulation)."""
    g = torch.Generator().manual_seed(24)
    shape, Cn = (4, 3, 24, 24), 3
    x = torch.randn(*shape, generator=g) + 100
    gamma, beta = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    dy = torch.randn(*shape, generator=g)

    def torch_bn(dtype):
        xs, gs, bs = (t.to(dtype).requires_grad_(True) for t in (x, gamma, beta))
        yy = F.batch_norm(xs, None, None, gs, bs, training=True, eps=1e-5)
        return yy.detach(), torch.autograd.grad(yy, [xs], dy.to(dtype))[0]

    y64, dx64 = torch_bn(torch.float64)
    y32, dx32 = torch_bn(torch.float32)
    ey_ref, edx_ref = rel_err(y32, y64), rel_err(dx32, dx64)
    xg, y, dx = x.to(gpu), torch.empty(shape, device=gpu), torch.empty(shape, device=gpu)
    dgam, dbet = torch.empty(Cn, device=gpu), torch.empty(Cn, device=gpu)
    saved = {}
    Kk.batchnorm_forward(xg, gamma.to(gpu), beta.to(gpu), y, False, 1e-5, saved)
    Kk.batchnorm_backward(xg, gamma.to(gpu), y, dy.to(gpu), dx, dgam, dbet, False, 1e-5, saved, False)
    ey, edx = rel_err(y.cpu(), y64), rel_err(dx.cpu(), dx64)
    print(f"bn offset: y err {ey:.3e} (torch fp32 {ey_ref:.3e}), dx err {edx:.3e} (torch fp32 {edx_ref:.3e})")
    assert ey <= 10 * ey_ref, (ey, ey_ref)
    assert edx <= 10 * edx_ref, (edx, edx_ref)
