"""permute, reverse, softmax and dropout (csrc/kernels/elementwise.hip) at the forms their first tests
left out: every permutation and axis, accumulation into a prefilled output, bf16, a strided input
view, sizes past 2048 blocks x 256 threads where the grid-stride loops start; softmax at awkward row
lengths, large and shifted logits and ``-inf`` entries; dropout's contract (no CPU oracle: the CPU path
draws from another generator, so the test checks values, rates, and that the mask is a function of
(seed, rank, step, index) alone -- every draw is a deterministic hash, so each assertion holds or
fails for good).  References are fp64 torch ops on the same (already rounded) inputs; copies are
compared exactly."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from flexmi.ops import _kernels as Kk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GRID_ELEMS = 2048 * 256       # elements one pass of the element-wise grid covers


def _rand(shape, dt, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dt).to(gpu)


def _add(a, b):
    """out (+)= v as the kernels compute it: one fp32 add, rounded once to the tensor's type."""
    return (a.float() + b.float()).to(a.dtype)


# ---------------------------------------------------------------- permute
PERMS = ([((5, 7, 11), p) for p in itertools.permutations(range(3))]
         + [((2, 3, 5, 7), (0, 2, 3, 1)), ((2, 5, 7, 3), (0, 3, 1, 2)),      # NCHW -> NHWC and back
            ((2, 3, 2, 5, 3, 4), (5, 2, 0, 4, 1, 3)), ((13, 9), (1, 0)), ((17,), (0,)),
            ((64, 96, 100), (2, 0, 1))])                                       # 614400 > GRID_ELEMS


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,perm", PERMS)
def test_permute(gpu, dt, shape, perm):
    x = _rand(shape, dt, gpu, 1)
    ref = x.permute(perm).contiguous()
    assert (ref.numel() > GRID_ELEMS) == (shape == (64, 96, 100))
    y = torch.full_like(ref, 3.0)
    Kk.permute(x, y, perm, False)
    assert torch.equal(y, ref)
    y0 = _rand(ref.shape, dt, gpu, 2)
    y = y0.clone()
    Kk.permute(x, y, perm, True)
    assert torch.equal(y, _add(y0, ref))


@pytest.mark.parametrize("dt", DTYPES)
def test_permute_strided_view(gpu, dt):
    base = _rand((6, 10, 7), dt, gpu, 3)
    x = base[:, ::2]                                  # (6, 5, 7), strides (70, 14, 1)
    assert not x.is_contiguous()
    for perm in ((2, 0, 1), (1, 2, 0)):
        ref = x.permute(perm).contiguous()
        y = torch.full_like(ref, 3.0)
        Kk.permute(x, y, perm, False)
        assert torch.equal(y, ref)


# ---------------------------------------------------------------- reverse
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,axis", [((3, 5, 7), 0), ((3, 5, 7), 1), ((3, 5, 7), 2), ((4, 1, 6), 1),
                                        ((9, 600, 100), 1)])                  # 540000 > GRID_ELEMS
def test_reverse(gpu, dt, shape, axis):
    x = _rand(shape, dt, gpu, 4)
    ref = x.flip(axis)
    y = torch.full_like(x, 3.0)
    Kk.reverse(x, y, axis, False)
    assert torch.equal(y, ref)
    y0 = _rand(shape, dt, gpu, 5)
    y = y0.clone()
    Kk.reverse(x, y, axis, True)
    assert torch.equal(y, _add(y0, ref))


# ---------------------------------------------------------------- softmax
def _softmax_check(x):
    """fp32: |y - ref| <= 1e-6.  bf16: one bf16 spacing of the result on top of that, 2^-8 ref + 1e-6.
    A row's sum is off 1 by at most the sum of its elements' bounds."""
    rows, C = x.shape
    y = torch.full_like(x, -1.0)
    Kk.softmax_forward(x, y)
    ref = torch.softmax(x.double(), -1)
    bound = 1e-6 + (2.0 ** -8) * ref if x.dtype == torch.bfloat16 else torch.full_like(ref, 1e-6)
    err = (y.double() - ref).abs()
    assert bool((err <= bound).all()), (err - bound).max().item()
    assert bool(((y.double().sum(-1) - 1).abs() <= bound.sum(-1)).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("form", ["unit", "x50", "shift1e4"])
@pytest.mark.parametrize("rows,C", [(5, 1), (5, 7), (5, 64), (5, 65), (5, 300), (5, 4099), (16400, 7)])
def test_softmax(gpu, dt, form, rows, C):
    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + rows))
    x = {"unit": x, "x50": x * 50, "shift1e4": x + 1e4}[form]
    _softmax_check(x.to(dt).to(gpu))


@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_neg_inf_entries(gpu, dt):
    x = torch.randn(5, 70, generator=torch.Generator().manual_seed(9))
    x[1, ::3] = float("-inf")
    x[2, 1:] = float("-inf")            # a single finite entry: the row is one-hot
    x[3, 64:] = float("-inf")           # the whole second pass of the wave
    _softmax_check(x.to(dt).to(gpu))


# ---------------------------------------------------------------- dropout
N = 1 << 20
RATE = 0.3
P_KEEP = 1 - RATE


def _ctx(rank=0, step=None):
    return SimpleNamespace(rank=rank, saved={} if step is None else {"step": step})


def _drop(x, seed, ctx, rate=RATE):
    y = torch.full_like(x, -1.0)
    Kk.dropout_forward(x, y, rate, seed, ctx)
    return y


@pytest.fixture(scope="module")
def drop_case(gpu):
    """One forward at (seed 11, rank 0, step 0) over n = 2^20 positive fp32 inputs, shared read-only."""
    x = torch.rand(N, generator=torch.Generator().manual_seed(0)).add_(0.5).to(gpu)
    y = _drop(x, 11, _ctx())
    return x, y, y != 0


def test_dropout_values_and_rate(drop_case):
    x, y, kept = drop_case
    keep = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(RATE))      # fp32, as the kernel
    exp = x * keep.item()
    assert bool(((y == 0) | ((y - exp).abs() <= 1e-6 * exp)).all())
    sigma = (RATE * P_KEEP / N) ** 0.5
    assert abs(kept.double().mean().item() - P_KEEP) <= 5 * sigma
    sigma = (RATE * P_KEEP / 1024) ** 0.5
    m = kept.view(1024, 1024).double()
    assert float((m.mean(1) - P_KEEP).abs().max()) <= 6 * sigma      # runs of consecutive indices
    assert float((m.mean(0) - P_KEEP).abs().max()) <= 6 * sigma      # indices 1024 apart


def test_dropout_mask_is_dtype_and_acc_independent(gpu, drop_case):
    x, y, kept = drop_case
    xb = x.bfloat16()
    yb = _drop(xb, 11, _ctx())
    assert torch.equal(yb != 0, kept)
    keep = 1.0 / (1.0 - torch.tensor(RATE).item())
    assert bool(((yb == 0) | ((yb.double() - xb.double() * keep).abs() <= 2.0 ** -8 * xb.double() * keep)).all())
    # the backward applies the forward's mask to dy (same seed, rank and saved step), acc or not
    dy = torch.rand(N, generator=torch.Generator().manual_seed(1)).add_(0.5).to(gpu)
    ctx = _ctx()
    _drop(x[:16], 11, ctx)
    assert ctx.saved["step"] == 0
    dx = torch.full_like(dy, -1.0)
    Kk.dropout_backward(dy, dx, RATE, 11, ctx, False)
    assert torch.equal(dx != 0, kept)
    base = torch.randn(N, generator=torch.Generator().manual_seed(2)).to(gpu)
    dxa = base.clone()
    Kk.dropout_backward(dy, dxa, RATE, 11, ctx, True)
    assert torch.equal(dxa != base, kept)
    torch.testing.assert_close(dxa, base + dx, rtol=1e-6, atol=1e-6)
    # bf16 accumulate: fp32 add, one rounding
    dyb, baseb = dy.bfloat16(), base.bfloat16()
    dxb = torch.full_like(dyb, -1.0)
    Kk.dropout_backward(dyb, dxb, RATE, 11, ctx, False)
    dxab = baseb.clone()
    Kk.dropout_backward(dyb, dxab, RATE, 11, ctx, True)
    assert torch.equal(dxb != 0, kept)
    exp = baseb.double() + dyb.double() * keep * kept
    assert bool(((dxab.double() - exp).abs() <= 2.0 ** -8 * exp.abs() + 1e-6).all())


def test_dropout_mask_depends_on_step_seed_rank(gpu, drop_case):
    x, y, kept = drop_case
    indep = 2 * RATE * P_KEEP            # share of positions where two independent masks differ
    for seed, ctx in ((11, _ctx(step=1)), (12, _ctx()), (11, _ctx(rank=1))):
        other = _drop(x, seed, ctx) != 0
        assert (other != kept).double().mean().item() >= 0.5 * indep, (seed, ctx)
        assert abs(other.double().mean().item() - P_KEEP) <= 5 * (RATE * P_KEEP / N) ** 0.5
    assert torch.equal(_drop(x, 11, _ctx(step=0)) != 0, kept)          # and on nothing else


def test_dropout_rate_zero_and_long_bf16(gpu, drop_case):
    x, y, kept = drop_case
    assert torch.equal(_drop(x, 11, _ctx(), rate=0.0), x)
    n = 2 * GRID_ELEMS + 4099            # past two passes of the grid, odd tail
    xb = torch.rand(n, generator=torch.Generator().manual_seed(3)).add_(0.5).bfloat16().to(gpu)
    yb = _drop(xb, 11, _ctx())
    kb = yb != 0
    assert torch.equal(kb[:N], kept)     # the mask is a function of the index
    assert abs(kb.double().mean().item() - P_KEEP) <= 5 * (RATE * P_KEEP / n) ** 0.5
    keep = 1.0 / (1.0 - torch.tensor(RATE).item())
    assert bool(((yb == 0) | ((yb.double() - xb.double() * keep).abs() <= 2.0 ** -8 * xb.double() * keep)).all())
