"""The LSTM cell kernels (csrc/kernels/lstm.hip: lstm_init, lstm_cell_fwd, lstm_cell_bwd) called
directly, with the strides flexmi/ops/rnn.py uses (batch-major [B, T, .] buffers, one step a strided
slice), against the cell equations in fp64.  Gate order i, f, g, o.

Every stored value is held to the fp64 value of its expression on the inputs the kernel had: the
activations against the pre-activations, c against the stored activations and c_prev, h against the
stored o and c.  Buffers are prefilled with a sentinel; everything outside step t must keep its bits.

Bounds, with s the sum of the magnitudes of the terms of an expression (|f c_prev| + |i g| for c;
the product of the factors' magnitudes and the sum bound of dc_t or dh_t for a gate gradient):
  * fp32 values: 2^-20 s.  Pre-activations lie in +-8, so the exponential amplifies the rounding of
    x log2(e) by at most 11.6 ulp, the divide and the products add a few: 16 ulp.
  * bf16 outputs (y, Hp, hT, cT, dG): 2^-8 s, one bf16 rounding.
  * the fp32 cell state keeps the fp32 bound in the bf16 runs.
In the backward c_t lies in +-1, where 1 - tanh(c)^2 amplifies tanhf's own last ulp by at most 3.6
(at |c| = 2 it is 27, past the 16 ulp the bound allows for the whole expression)."""
import pytest
import torch

from flexmi.ops import _kernels as Kk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(1, 1), (3, 5), (7, 33), (64, 64)]
BIG = (257, 2049)             # 526593 elements: past the 524288 of one pass of the grid
T = 3
SENT = -777.0
F32, BF16 = 2.0 ** -20, 2.0 ** -8


def _uni(shape, lo, hi, seed, dt=torch.float32):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo).to(dt)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _within(got, ref, s, tol, what):
    got = got.cpu().double()
    assert not torch.isnan(got).any(), what
    err = (got - ref).abs()
    assert bool((err <= tol * s).all()), (what, (err / s.clamp_min(1e-300)).max().item(), tol)


def _others_kept(buf, t, what):
    """buf [B, T, W] was filled with SENT: every step but t still holds it, bit for bit."""
    keep = [u for u in range(T) if u != t]
    ref = torch.full_like(buf[:, keep], SENT)
    assert torch.equal(_bits(buf[:, keep]), _bits(ref)), what


def _forward_case(gpu, B, H, dt, t, give_next, give_final):
    tol = BF16 if dt == torch.bfloat16 else F32
    pre = _uni((B, 4 * H), -8.0, 8.0, 1)
    cprev = _uni((B, H), -2.0, 2.0, 2)
    G = torch.full((B, T, 4 * H), SENT)
    G[:, t] = pre
    Cs = torch.full((B, T, H), SENT)
    cinit = torch.full((B, H), SENT)
    if t == 0:
        cinit.copy_(cprev)
    else:
        Cs[:, t - 1] = cprev
    G, Cs, cinit = G.to(gpu), Cs.to(gpu), cinit.to(gpu)
    y = torch.full((B, T, H), SENT, dtype=dt, device=gpu)
    Hp = torch.full((B, T, H), SENT, dtype=dt, device=gpu)
    hT = torch.full((B, H), SENT, dtype=dt, device=gpu) if give_final else None
    cT = torch.full((B, H), SENT, dtype=dt, device=gpu) if give_final else None
    cp, cp_off, ldcp = (cinit, 0, H) if t == 0 else (Cs, (t - 1) * H, T * H)
    Kk.C().lstm_cell_fwd(G.view(-1), t * 4 * H, T * 4 * H, cp.view(-1), cp_off, ldcp, Cs.view(-1), t * H, T * H,
                         y.view(-1), t * H, T * H, Hp.view(-1), (t + 1) * H if give_next else -1, T * H, hT, cT, B, H)
    what = ("fwd", B, H, dt, t, give_next, give_final)
    # activations against the pre-activations
    pd = pre.double()
    act = torch.cat([torch.sigmoid(pd[:, :2 * H]), torch.tanh(pd[:, 2 * H:3 * H]), torch.sigmoid(pd[:, 3 * H:])], 1)
    _within(G[:, t], act, act.abs(), F32, what + ("G",))
    _others_kept(G, t, what + ("G",))
    # c against the stored activations
    a = G[:, t].cpu().double()
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    cd = cprev.double()
    _within(Cs[:, t], f * cd + i * g, (f * cd).abs() + (i * g).abs(), F32, what + ("c",))
    keep = [u for u in range(T) if u != t and not (t > 0 and u == t - 1)]
    assert torch.equal(_bits(Cs[:, keep]), _bits(torch.full_like(Cs[:, keep], SENT))), what
    if t > 0:
        assert torch.equal(Cs[:, t - 1].cpu(), cprev), what
    else:
        assert torch.equal(cinit.cpu(), cprev), what
    # h against the stored o and c
    c = Cs[:, t].cpu().double()
    h = o * torch.tanh(c)
    _within(y[:, t], h, h.abs(), tol, what + ("y",))
    _others_kept(y, t, what + ("y",))
    if give_next:
        assert torch.equal(_bits(Hp[:, t + 1]), _bits(y[:, t])), what
        _others_kept(Hp, t + 1, what + ("Hp",))
    else:
        assert torch.equal(_bits(Hp), _bits(torch.full_like(Hp, SENT))), what
    if give_final:
        assert torch.equal(_bits(hT), _bits(y[:, t])), what
        _within(cT, c, c.abs(), tol, what + ("cT",))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H", SHAPES)
def test_cell_forward(gpu, B, H, dt):
    _forward_case(gpu, B, H, dt, 1, True, False)        # a middle step: c_prev from Cs, Hp for the next
    _forward_case(gpu, B, H, dt, 0, True, True)         # the first step: c_prev from cinit
    _forward_case(gpu, B, H, dt, 1, False, True)        # as the last step: no Hp, hT and cT
    _forward_case(gpu, B, H, dt, 0, False, False)


def _backward_case(gpu, B, H, dt, t, give_dy):
    tol = BF16 if dt == torch.bfloat16 else F32
    pre = _uni((B, 4 * H), -8.0, 8.0, 3)
    act = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])], 1)
    ct, cprev = _uni((B, H), -1.0, 1.0, 4), _uni((B, H), -2.0, 2.0, 5)
    dh0, dc0 = _uni((B, H), -1.0, 1.0, 6), _uni((B, H), -1.0, 1.0, 7)
    dy0 = _uni((B, H), -1.0, 1.0, 8, dt)
    A = torch.full((B, T, 4 * H), SENT)
    A[:, t] = act
    Cs = torch.full((B, T, H), SENT)
    Cs[:, t] = ct
    cinit = torch.full((B, H), SENT)
    if t == 0:
        cinit.copy_(cprev)
    else:
        Cs[:, t - 1] = cprev
    dy = torch.full((B, T, H), SENT, dtype=dt)
    dy[:, t] = dy0
    A, Cs, cinit, dy = A.to(gpu), Cs.to(gpu), cinit.to(gpu), dy.to(gpu)
    dh, dc = dh0.to(gpu), dc0.to(gpu)
    dG = torch.full((B, T, 4 * H), SENT, dtype=dt, device=gpu)
    cp, cp_off, ldcp = (cinit, 0, H) if t == 0 else (Cs, (t - 1) * H, T * H)
    Kk.C().lstm_cell_bwd(A.view(-1), t * 4 * H, T * 4 * H, Cs.view(-1), t * H, T * H, cp.view(-1), cp_off, ldcp,
                         dy.view(-1) if give_dy else None, t * H, T * H, dh.view(-1), dc.view(-1),
                         dG.view(-1), t * 4 * H, T * 4 * H, B, H)
    what = ("bwd", B, H, dt, t, give_dy)
    a = act.double()
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    tc, cpd = torch.tanh(ct.double()), cprev.double()
    dyd = dy0.double() if give_dy else torch.zeros(B, H, dtype=torch.float64)
    dht, s_dht = dh0.double() + dyd, dh0.double().abs() + dyd.abs()
    k = o * (1 - tc * tc)
    dct, s_dct = dc0.double() + dht * k, dc0.double().abs() + s_dht * k
    gates = [(dct * g * i * (1 - i), s_dct * (g * i * (1 - i)).abs()),
             (dct * cpd * f * (1 - f), s_dct * (cpd * f * (1 - f)).abs()),
             (dct * i * (1 - g * g), s_dct * (i * (1 - g * g)).abs()),
             (dht * tc * o * (1 - o), s_dht * (tc * o * (1 - o)).abs())]
    for q, (ref, s) in enumerate(gates):
        _within(dG[:, t, q * H:(q + 1) * H], ref, s, tol, what + ("dG", "ifgo"[q]))
    _others_kept(dG, t, what + ("dG",))
    _within(dc, dct * f, s_dct * f, F32, what + ("dc",))
    assert torch.equal(dh.cpu(), dh0), what              # read only


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H", SHAPES)
def test_cell_backward(gpu, B, H, dt):
    for t in (1, 0):
        for give_dy in (True, False):
            _backward_case(gpu, B, H, dt, t, give_dy)


@pytest.mark.parametrize("dt", DTYPES)
def test_cell_past_one_grid_pass(gpu, dt):
    B, H = BIG
    assert B * H > 2048 * 256
    _forward_case(gpu, B, H, dt, 1, True, True)
    _backward_case(gpu, B, H, dt, 1, True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H", SHAPES)
def test_lstm_init(gpu, B, H, dt):
    h0, c0 = _uni((B, H), -1.0, 1.0, 9, dt), _uni((B, H), -2.0, 2.0, 10, dt)
    for given in (True, False):
        Hp = torch.full((B, T, H), SENT, dtype=dt, device=gpu)
        cinit = torch.full((B, H), SENT, device=gpu)
        Kk.C().lstm_init(h0.to(gpu) if given else None, c0.to(gpu) if given else None, Hp.view(-1), T * H,
                         cinit.view(-1), B, H)
        assert torch.equal(_bits(Hp[:, 0]), _bits(h0 if given else torch.zeros_like(h0))), (B, H, dt, given)
        assert torch.equal(_bits(cinit), _bits(c0.float() if given else torch.zeros(B, H))), (B, H, dt, given)
        _others_kept(Hp, 0, ("init", B, H, dt, given))


# ---------------------------------------------------------------- binding checks (nothing is launched)
def test_lstm_bindings_refuse_wrong_dtypes(gpu):
    B, H = 2, 4
    C = Kk.C()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=gpu)      # noqa: E731
    bf, f16 = torch.bfloat16, torch.float16

    def fwd(G=None, cp=None, Cs=None, y=None, Hp=None, hT=None, cT=None):
        C.lstm_cell_fwd(z(B * T * 4 * H) if G is None else G, 0, T * 4 * H, z(B * H) if cp is None else cp, 0, H,
                        z(B * T * H) if Cs is None else Cs, 0, T * H, z(B * T * H) if y is None else y, 0, T * H,
                        z(B * T * H) if Hp is None else Hp, H, T * H, hT, cT, B, H)

    def bwd(A=None, Cs=None, cp=None, dy=None, dh=None, dc=None, dG=None):
        C.lstm_cell_bwd(z(B * T * 4 * H) if A is None else A, 0, T * 4 * H, z(B * T * H) if Cs is None else Cs, 0, T * H,
                        z(B * H) if cp is None else cp, 0, H, dy, 0, T * H, z(B * H) if dh is None else dh,
                        z(B * H) if dc is None else dc, z(B * T * 4 * H) if dG is None else dG, 0, T * 4 * H, B, H)

    fwd(hT=z(B * H), cT=z(B * H))                       # the forms themselves are accepted
    bwd(dy=z(B * T * H))
    for kw in (dict(G=z(B * T * 4 * H, bf)), dict(cp=z(B * H, bf)), dict(Cs=z(B * T * H, bf)), dict(y=z(B * T * H, f16)),
               dict(Hp=z(B * T * H, bf)), dict(hT=z(B * H, bf)), dict(cT=z(B * H, bf)), dict(y=z(B * T * H, bf)),
               dict(y=torch.zeros(B * T * H)), dict(hT=z(B * H - 1))):
        with pytest.raises(RuntimeError):
            fwd(**kw)
    for kw in (dict(A=z(B * T * 4 * H, bf)), dict(Cs=z(B * T * H, bf)), dict(cp=z(B * H, bf)), dict(dy=z(B * T * H, bf)),
               dict(dh=z(B * H, bf)), dict(dc=z(B * H, bf)), dict(dG=z(B * T * 4 * H, f16)), dict(dc=z(B * H - 1))):
        with pytest.raises(RuntimeError):
            bwd(**kw)
    for kw in (dict(h0=z(B * H, bf)), dict(c0=z(B * H, bf)), dict(cinit=z(B * H, bf)), dict(hprev=z(B * T * H, f16)),
               dict(h0=z(B * H - 1))):
        a = dict(h0=z(B * H), c0=z(B * H), hprev=z(B * T * H), cinit=z(B * H))
        a.update(kw)
        with pytest.raises(RuntimeError):
            C.lstm_init(a["h0"], a["c0"], a["hprev"], T * H, a["cinit"], B, H)
