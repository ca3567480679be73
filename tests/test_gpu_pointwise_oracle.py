"""Unary and binary element-wise kernels (csrc/kernels/elementwise.hip: fm_unary_fwd/bwd,
fm_binary_fwd/bwd) against fp64 oracles, on every dispatch path, and the gradient of an op that
reads one tensor at two inputs on the HIP backend.

Inputs are drawn on the CPU from a seeded generator and rounded to the storage type; the oracle is
plain torch in fp64 on those rounded inputs.  Sizes: 1 and 7 (scalar tail only), 8 (one vector
iteration, no tail), 2053 (vector plus a 5-element tail) and 2048*256*8 + 8*300 + 5 (past one pass of
the grid, so the grid-stride loop runs, and a tail follows).  Alignment: all operands 16-B aligned;
every operand a view one element in; only the output, or only one input, one element in -- the
launcher must then take the scalar path as a whole.  Every output view has spare elements before and
after it which must keep their bits.

Bounds, with s the magnitude of the result (with accumulation: of the new term plus the prefilled
value it is added to):
  * relu, relu backward, add, sub and plain copies of the gradient: equal to the fp32 computation
    rounded once to the storage type (one IEEE operation; -0 and +0 compare equal).
  * fp32, |x| <= 8: |got - ref| <= 2^-20 s.  The hardware exp2 / log2 is good to about 1 ulp; the fp32
    multiply by log2(e) in front of it has half an ulp of its own, which the exponential amplifies by
    |x| log2(e) <= 11.6; the divide of the sigmoid, or the three roundings of -g u / (v v), add a few
    more: 16 ulp = 2^-20.  tanh backward computes 1 - y*y with one rounding (fmaf): in two roundings
    the result is lost where |y| -> 1, and the bound would not hold.
  * fp32, x over +-80 (sigmoid, tanh, exp): the same with 2^-16 (the amplification is 115), no NaN.
  * bf16: |got - ref| <= 2^-8 s, one bf16 rounding of a value the fp32 arithmetic placed within
    2^-20 of the truth (half a bf16 ulp is at most 2^-8 of the value; the bound at a rounding midpoint
    exceeds it by 2^-16 s, which covers the fp32 error).
  * ELU: inputs include -logspace(-7, 0), where exp(x) - 1 in fp32 is 22 % off; expm1f keeps 2^-20."""
import itertools

import pytest
import torch

from flexmi.ops import _kernels as Kk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SMALL = [1, 7, 8, 2053]
BIG = 2048 * 256 * 8 + 8 * 300 + 5
ALIGN = ["aligned", "all_off1", "out_off1", "in_off1"]
F32, BF16 = 2.0 ** -20, 2.0 ** -8


def _tol(dt):
    return BF16 if dt == torch.bfloat16 else F32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uni(n, lo, hi, seed, dt):
    return (torch.rand(n, generator=_gen(seed)) * (hi - lo) + lo).to(dt)


def _randn(n, seed, dt):
    return torch.randn(n, generator=_gen(seed)).to(dt)


class Slot:
    """A CPU tensor placed ``off`` elements into a device buffer with one spare element after it."""

    def __init__(self, t, gpu, off):
        n = t.numel()
        buf = torch.full((off + n + 1,), -777.0, dtype=t.dtype)
        buf[off:off + n] = t
        self.n, self.off, self.snap = n, off, buf.clone()
        self.buf = buf.to(gpu)
        self.view = self.buf[off:off + n]
        assert self.view.data_ptr() % 16 == (off * t.element_size()) % 16

    def guards_kept(self):
        it = torch.int32 if self.snap.dtype == torch.float32 else torch.int16
        now, was = self.buf.cpu().view(it), self.snap.view(it)
        e = self.off + self.n
        return torch.equal(now[:self.off], was[:self.off]) and torch.equal(now[e:], was[e:])


def _offs(align, nin):
    """(input offsets, output offset) of a form; 'in_off1' misaligns the last input only."""
    if align == "aligned":
        return [0] * nin, 0
    if align == "all_off1":
        return [1] * nin, 1
    if align == "out_off1":
        return [0] * nin, 1
    return [0] * (nin - 1) + [1], 0


def _check(got, ref, s, tol, what):
    got = got.cpu().double()
    assert not torch.isnan(got).any(), what
    err = (got - ref).abs()
    bound = tol * s
    assert bool((err <= bound).all()), (what, ((err - bound) / s.clamp_min(1e-300)).max().item(), tol)


# ---------------------------------------------------------------- unary
def _unary_x(code, n, dt, lo=-8.0, hi=8.0):
    x = _uni(n, lo, hi, 100 + code, torch.float32)
    if n > 16:
        x[3] = 0.0
    if code == 3 and n >= 2053:
        x[:96] = -torch.logspace(-7, 0, 96)          # the vector path
        x[-5:] = -torch.logspace(-7, -3, 5)          # the scalar tail
    return x.to(dt)


def _unary_ref(code, x):
    """fp64 forward of the (rounded) x."""
    x = x.double()
    return [torch.relu(x), torch.sigmoid(x), torch.tanh(x), torch.where(x > 0, x, torch.expm1(x)), torch.exp(x)][code]


def _unary_fwd_case(gpu, code, dt, n, align, tol=None, x=None):
    x = _unary_x(code, n, dt) if x is None else x
    (ox,), oy = _offs(align, 1)
    sx, sy = Slot(x, gpu, ox), Slot(_randn(n, 1, dt), gpu, oy)
    Kk.C().unary_fwd(code, sx.view, sy.view)
    ref = _unary_ref(code, x)
    what = ("unary_fwd", code, dt, n, align)
    if code == 0:
        assert torch.equal(sy.view.cpu(), torch.relu(x)), what
    else:
        _check(sy.view, ref, ref.abs(), tol or _tol(dt), what)
    assert sy.guards_kept() and torch.equal(sx.buf.cpu(), sx.snap), what


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("code", range(5))
def test_unary_forward(gpu, code, dt):
    for n, align in itertools.product(SMALL, ALIGN):
        _unary_fwd_case(gpu, code, dt, n, align)


@pytest.mark.parametrize("code", [1, 2, 4])
def test_unary_forward_wide_fp32(gpu, code):
    x = _uni(2053, -80.0, 80.0, 7, torch.float32)
    for align in ("aligned", "all_off1"):
        _unary_fwd_case(gpu, code, torch.float32, 2053, align, tol=2.0 ** -16, x=x)


def test_unary_saturation(gpu):
    x = torch.tensor([-100.0, 100.0] * 8 + [-100.0, 100.0, 100.0])      # 16 vector + 3 tail elements
    for dt in DTYPES:
        xs = x.to(dt).to(gpu)
        y = torch.empty_like(xs)
        Kk.C().unary_fwd(1, xs, y)
        y = y.cpu().double()
        assert bool((y[x < 0] >= 0).all()) and bool((y[x < 0] <= 1e-37).all()) and bool((y[x > 0] == 1).all())
        y = torch.empty_like(xs)
        Kk.C().unary_fwd(2, xs, y)
        assert torch.equal(y.cpu().double(), torch.sign(x).double())


def _unary_bwd_case(gpu, code, dt, n, align, acc):
    x = _unary_x(code, n, dt)
    y = _unary_ref(code, x).to(dt)                 # what the forward stored
    dy, dx0 = _randn(n, 2, dt), _randn(n, 3, dt)
    offs, od = _offs(align, 3)
    sx, sy, sdy = (Slot(t, gpu, o) for t, o in zip((x, y, dy), offs))
    sdx = Slot(dx0, gpu, od)
    Kk.C().unary_bwd(code, sx.view, sy.view, sdy.view, sdx.view, acc)
    xd, yd, g = x.double(), y.double(), dy.double()
    term = [torch.where(xd > 0, g, torch.zeros_like(g)), g * yd * (1 - yd), g * (1 - yd * yd),
            torch.where(xd > 0, g, g * (yd + 1)), g * yd][code]
    what = ("unary_bwd", code, dt, n, align, acc)
    if code == 0:
        t32 = torch.where(x > 0, dy, torch.zeros_like(dy)).float()
        assert torch.equal(sdx.view.cpu(), ((t32 + dx0.float()) if acc else t32).to(dt)), what
    else:
        ref, s = (term + dx0.double(), term.abs() + dx0.double().abs()) if acc else (term, term.abs())
        _check(sdx.view, ref, s, _tol(dt), what)
    assert sdx.guards_kept(), what


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("code", range(5))
def test_unary_backward(gpu, code, dt, acc):
    for n, align in itertools.product(SMALL, ALIGN):
        _unary_bwd_case(gpu, code, dt, n, align, acc)


# ---------------------------------------------------------------- binary
def _binary_ab(code, n, dt):
    a = _uni(n, -4.0, 4.0, 10, dt)
    b = _uni(n, -4.0, 4.0, 11, dt)
    if code == 3:                                   # +-[0.5, 2]
        sign = torch.where(torch.rand(n, generator=_gen(12)) < 0.5, -1.0, 1.0)
        b = (sign * _uni(n, 0.5, 2.0, 13, torch.float32)).to(dt)
    return a, b


def _binary_fwd_case(gpu, code, dt, n, align, relu):
    a, b = _binary_ab(code, n, dt)
    offs, oy = _offs(align, 2)
    sa, sb = Slot(a, gpu, offs[0]), Slot(b, gpu, offs[1])
    sy = Slot(_randn(n, 1, dt), gpu, oy)
    Kk.C().binary_fwd(code, sa.view, sb.view, sy.view, relu)
    what = ("binary_fwd", code, dt, n, align, relu)
    if code < 2:
        r32 = a.float() + b.float() if code == 0 else a.float() - b.float()
        assert torch.equal(sy.view.cpu(), (torch.relu(r32) if relu else r32).to(dt)), what
    else:
        ref = a.double() * b.double() if code == 2 else a.double() / b.double()
        ref = torch.relu(ref) if relu else ref
        _check(sy.view, ref, ref.abs(), _tol(dt), what)
    assert sy.guards_kept(), what


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("code", range(4))
def test_binary_forward(gpu, code, dt, relu):
    for n, align in itertools.product(SMALL, ALIGN):
        _binary_fwd_case(gpu, code, dt, n, align, relu)


OUTS = [("da", "db"), ("da",), ("db",)]


def _binary_bwd_case(gpu, code, dt, n, align, masked, outs, acca, accb):
    a, b = _binary_ab(code, n, dt)
    dy = _randn(n, 2, dt)
    m = _randn(n, 4, dt)
    if n > 16:
        m[5] = 0.0                                  # y == 0 passes nothing
    pre = {"da": _randn(n, 5, dt), "db": _randn(n, 6, dt)}
    nin = 4 if masked else 3
    offs, oo = _offs(align, nin)
    sa, sb, sdy = Slot(a, gpu, offs[0]), Slot(b, gpu, offs[1]), Slot(dy, gpu, offs[2])
    sm = Slot(m, gpu, offs[3]) if masked else None
    so = {k: Slot(pre[k], gpu, oo) for k in outs}
    Kk.C().binary_bwd(code, sa.view, sb.view, sdy.view, sm.view if masked else None,
                      so["da"].view if "da" in so else None, so["db"].view if "db" in so else None, acca, accb)
    g = torch.where(m > 0, dy, torch.zeros_like(dy)) if masked else dy
    gd, u, v = g.double(), a.double(), b.double()
    terms = {"da": [gd, gd, gd * v, gd / v][code], "db": [gd, -gd, gd * u, -gd * u / (v * v)][code]}
    for k, acc in (("da", acca), ("db", accb)):
        if k not in so:
            continue
        what = ("binary_bwd", code, dt, n, align, masked, outs, acca, accb, k)
        p = pre[k]
        if code < 2:
            t32 = (-g if (code == 1 and k == "db") else g).float()
            assert torch.equal(so[k].view.cpu(), ((t32 + p.float()) if acc else t32).to(dt)), what
        else:
            t = terms[k]
            ref, s = (t + p.double(), t.abs() + p.double().abs()) if acc else (t, t.abs())
            _check(so[k].view, ref, s, _tol(dt), what)
        assert so[k].guards_kept(), what


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("code", range(4))
def test_binary_backward(gpu, code, dt, masked):
    for outs in OUTS:
        for acca, accb in itertools.product([False, True], repeat=2):
            if ("da" not in outs and acca) or ("db" not in outs and accb):
                continue
            for n, align in itertools.product(SMALL, ALIGN):
                _binary_bwd_case(gpu, code, dt, n, align, masked, outs, acca, accb)


# ---------------------------------------------------------------- past one pass of the grid
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kernel", ["unary_fwd", "unary_bwd", "binary_fwd", "binary_bwd"])
def test_grid_stride(gpu, kernel, dt):
    assert BIG == 4196709 and BIG // 8 > 2048 * 256 and BIG % 8 == 5
    if kernel == "unary_fwd":
        _unary_fwd_case(gpu, 3, dt, BIG, "aligned")
    elif kernel == "unary_bwd":
        _unary_bwd_case(gpu, 1, dt, BIG, "aligned", True)
    elif kernel == "binary_fwd":
        _binary_fwd_case(gpu, 3, dt, BIG, "aligned", False)
    else:
        _binary_bwd_case(gpu, 3, dt, BIG, "aligned", True, ("da", "db"), True, True)


# ---------------------------------------------------------------- binding checks (nothing is launched)
def test_bindings_refuse_bad_operands(gpu):
    C = Kk.C()
    ok = lambda dt=torch.float32, n=16: torch.zeros(n, dtype=dt, device=gpu)       # noqa: E731
    strided = torch.zeros(32, device=gpu)[::2]
    bad = [("non-contiguous", strided), ("other dtype", ok(torch.bfloat16)), ("other size", ok(n=17)),
           ("host tensor", torch.zeros(16))]
    for what, t in bad:
        for pos in range(2):
            args = [ok(), ok()]
            args[pos] = t
            with pytest.raises(RuntimeError):
                C.unary_fwd(1, *args)
        for pos in range(1, 4):
            args = [ok(), ok(), ok(), ok()]
            args[pos] = t
            with pytest.raises(RuntimeError):
                C.unary_bwd(1, *args, False)
        for pos in range(1, 3):
            args = [ok(), ok(), ok()]
            args[pos] = t
            with pytest.raises(RuntimeError):
                C.binary_fwd(2, *args, False)
        for pos in range(1, 6):
            args = [ok(), ok(), ok(), ok(), ok(), ok()]
            args[pos] = t
            with pytest.raises(RuntimeError):
                C.binary_bwd(2, *args, False, False)
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(RuntimeError):
            C.unary_fwd(0, ok(dt), ok(dt))
        with pytest.raises(RuntimeError):
            C.unary_bwd(0, ok(dt), ok(dt), ok(dt), ok(dt), False)
        with pytest.raises(RuntimeError):
            C.binary_fwd(0, ok(dt), ok(dt), ok(dt), False)
        with pytest.raises(RuntimeError):
            C.binary_bwd(0, ok(dt), ok(dt), ok(dt), None, ok(dt), None, False, False)
    with pytest.raises(RuntimeError):
        C.unary_fwd(0, strided, ok())
    with pytest.raises(RuntimeError):
        C.binary_fwd(0, strided, ok(), ok(), False)


# ---------------------------------------------------------------- one tensor at two inputs, HIP backend
@pytest.mark.parametrize("form", ["multiply", "add", "subtract", "relu_add"])
def test_dup_input_grad_gpu(gpu, form):
    """tests/test_dup_input_grad_cpu.py on the HIP backend (fp32 compute); 'relu_add' takes the
    executor's fused add + ReLU, whose backward passes the ReLU output as ymask."""
    from tests.test_dup_input_grad_cpu import check_dup_case
    check_dup_case(form, "gpu")
