"""The dense update rules on MI355X (csrc/kernels/update_rule.h): every rule through the one
traversal -- scalar head up to the 16-B boundary, 16-B body, scalar tail -- against a float64 torch
oracle, and bit-identical whatever the split into head, body and tail is.

Sizes 1, 3, 4, 5, 8, 11, 1031 at element offsets 0..3 into 16-B aligned allocations are the smallest
that give an empty head, a head only, one vector, head + vector + tail and a multi-block body.
Tolerances are those of tests/test_gpu_adagrad.py (rtol 1e-5, atol 1e-6) and
tests/test_gpu_kernels.py::test_sgd_adam (SGD atol 1e-5, Adam W atol 1e-4; allclose's rtol 1e-5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 8, 11, 1031)
NMAX, PAD = max(NS), 8
STEP, EPS = 0.05, 1e-8
FILL = 7.0          # what the buffers hold outside the updated range

# name -> (kind, constants, state names): SGD (wd, mom, nesterov); Adagrad (wd, eps); Adam (b1, b2, wd, eps)
RULES = {
    "sgd": ("sgd", (0.0, 0.0, False), ()),
    "sgd_nesterov_wd": ("sgd", (1e-3, 0.9, True), ("v",)),
    "adagrad": ("adagrad", (0.0, 1e-10), ("h",)),
    "adagrad_wd": ("adagrad", (1e-3, 1e-10), ("h",)),
    "adam": ("adam", (0.9, 0.999, 1e-3, EPS), ("m", "v")),
}
# (rtol, atol) of W and of the state, per kind
TOL = {"sgd": ((1e-5, 1e-5), (1e-5, 1e-5)), "adagrad": ((1e-5, 1e-6), (1e-5, 1e-6)), "adam": ((1e-5, 1e-4), (1e-5, 1e-5))}


def _values(kind, names, dev):
    """One seeded set of NMAX values: w, g and the states (accumulators of squares in [0.1, 1):
    the update is ill-conditioned at 0, tests/test_gpu_adagrad.py)."""
    gen = torch.Generator().manual_seed(11)
    w, g = torch.randn(NMAX, generator=gen).to(dev), torch.randn(NMAX, generator=gen).to(dev)
    st = []
    for nm in names:
        sq = nm == "h" or (kind == "adam" and nm == "v")
        st.append((torch.rand(NMAX, generator=gen) * 0.9 + 0.1 if sq else torch.randn(NMAX, generator=gen)).to(dev))
    return w, g, st


def _oracle(kind, c, w, g, st):
    """float64 rule -> (w, states)."""
    w, g, st = w.double(), g.double(), [s.double() for s in st]
    if kind == "sgd":
        wd, mom, nest = c
        g = g + wd * w
        if mom > 0:
            st = [mom * st[0] + g]
            g = g + mom * st[0] if nest else st[0]
        return w - STEP * g, st
    if kind == "adagrad":
        wd, eps = c
        g = g + wd * w
        h = st[0] + g * g
        return w - STEP * g / (h.sqrt() + eps), [h]
    b1, b2, wd, eps = c
    g = g + wd * w
    m, v = b1 * st[0] + (1 - b1) * g, b2 * st[1] + (1 - b2) * g * g
    return w - STEP * m / (v.sqrt() + eps), [m, v]


def _launch(kind, c, W, G, S, Wc, step, zero_grad):
    from flexmi.ops import _kernels as K
    if kind == "sgd":
        K.sgd_update(W, G, S[0] if S else None, Wc, step, *c, zero_grad=zero_grad)
    elif kind == "adagrad":
        K.adagrad_update(W, G, S[0], Wc, step, *c, zero_grad=zero_grad)
    else:
        K.adam_update(W, G, S[0], S[1], Wc, step, *c, zero_grad=zero_grad)


def _placed(vals, n, off, dtype=torch.float32):
    """A 16-B aligned allocation of FILL with vals[:n] at element offset off -> (buffer, view)."""
    buf = torch.full((n + PAD,), FILL, device=vals.device, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n] = vals[:n]
    return buf, buf[off:off + n]


def _run(kind, c, vals, n, off, mirror, zero_grad, step, g_off=None):
    """The rule over views ``off`` elements into their buffers (G: ``g_off``) -> (W, states, mirror, G) views
    after asserting (c) nothing outside the views was written and (d) G is zero / unchanged."""
    w, g, st = vals
    bufs = [_placed(w, n, off), _placed(g, n, off if g_off is None else g_off)] + [_placed(s, n, off) for s in st]
    cb = _placed(torch.full((NMAX,), FILL, device=w.device), n, off, torch.bfloat16)
    _launch(kind, c, bufs[0][1], bufs[1][1], [b[1] for b in bufs[2:]], cb[1] if mirror else None, step, zero_grad)
    for (buf, view), o in zip(bufs + [cb], [off, off if g_off is None else g_off] + [off] * (len(st) + 1)):
        assert int((buf[:o] != FILL).sum()) == 0 and int((buf[o + n:] != FILL).sum()) == 0, (n, off, "outside the range")
    G = bufs[1][1]
    assert int((G != 0).sum()) == 0 if zero_grad else torch.equal(G, g[:n]), (n, off, "G")
    if not mirror:
        assert int((cb[0] != FILL).sum()) == 0
    return bufs[0][1], [b[1] for b in bufs[2:]], cb[1] if mirror else None


def _check_oracle(kind, c, vals, n, W, S):
    w64, s64 = _oracle(kind, c, vals[0][:n], vals[1][:n], [s[:n] for s in vals[2]])
    (wr, wa), (sr, sa) = TOL[kind]
    torch.testing.assert_close(W.double(), w64, rtol=wr, atol=wa)
    for s, r in zip(S, s64):
        torch.testing.assert_close(s.double(), r, rtol=sr, atol=sa)


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("rule", list(RULES))
def test_rule_at_every_size_and_offset(gpu, rule, mirror, zero_grad):
    kind, c, names = RULES[rule]
    vals = _values(kind, names, gpu)
    step = torch.tensor([STEP], device=gpu)
    for n in NS:
        ref = None
        for off in range(4):
            W, S, Wc = _run(kind, c, vals, n, off, mirror, zero_grad, step)
            _check_oracle(kind, c, vals, n, W, S)                      # (a)
            if mirror:
                assert torch.equal(Wc, W.bfloat16())
            if ref is None:
                ref = (W, S, Wc)
                continue
            # (b) head, body and tail are the same arithmetic: the split does not change a bit
            assert torch.equal(W, ref[0]) and all(torch.equal(a, b) for a, b in zip(S, ref[1])), (n, off)
            assert not mirror or torch.equal(Wc, ref[2]), (n, off)
    # G one element off against W: not congruent modulo 16 B, so every element goes scalar
    n = NMAX
    W, S, Wc = _run(kind, c, vals, n, 0, mirror, zero_grad, step, g_off=1)
    _check_oracle(kind, c, vals, n, W, S)
    assert torch.equal(W, ref[0]) and all(torch.equal(a, b) for a, b in zip(S, ref[1]))
    assert not mirror or torch.equal(Wc, ref[2])


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("rule", ["sgd", "sgd_nesterov_wd"])
def test_sgd_segs_is_sgd_update_bit_for_bit(gpu, rule, mirror, zero_grad):
    """Every (size, offset mod 4) as one range of ONE segmented launch over 16-B aligned flat
    buffers, against the flat launch on the same values."""
    from flexmi.ops import _kernels as K
    kind, c, names = RULES[rule]
    vals = _values(kind, names, gpu)
    w, g, st = vals
    step = torch.tensor([STEP], device=gpu)
    segs, at = [], 0
    for n in NS:
        for off in range(4):
            at = (at + 4) // 4 * 4 + off      # a gap of >= 1 element, start = off mod 4
            segs.append((at, n))
            at += n
    total = at + PAD
    flat = [torch.full((total,), FILL, device=gpu) for _ in range(2 + len(st))]
    Cb = torch.full((total,), FILL, device=gpu, dtype=torch.bfloat16)
    inside = torch.zeros(total, dtype=torch.bool, device=gpu)
    for o, n in segs:
        for buf, v in zip(flat, [w, g] + st):
            buf[o:o + n] = v[:n]
        inside[o:o + n] = True
    K.C().sgd_segs(flat[0], flat[1], flat[2] if st else None, Cb if mirror else None, step, [s[0] for s in segs],
                   [s[1] for s in segs], *c, zero_grad)
    for buf in flat + [Cb]:
        assert int((buf[~inside] != FILL).sum()) == 0                 # (c)
    if not mirror:
        assert int((Cb != FILL).sum()) == 0
    for n in NS:
        W, S, Wc = _run(kind, c, vals, n, 0, mirror, zero_grad, step)
        for o, m in segs:
            if m != n:
                continue
            assert torch.equal(flat[0][o:o + n], W) and all(torch.equal(flat[2][o:o + n], s) for s in S), (o, n)
            assert not mirror or torch.equal(Cb[o:o + n], Wc), (o, n)
            G = flat[1][o:o + n]
            assert int((G != 0).sum()) == 0 if zero_grad else torch.equal(G, g[:n]), (o, n)      # (d)


@pytest.mark.parametrize("bad", ["dtype", "short_state", "cpu_step", "short_mirror"])
@pytest.mark.parametrize("entry", ["sgd", "sgd_segs", "adam", "adagrad"])
def test_malformed_arguments_raise_without_launching(gpu, entry, bad):
    from flexmi.ops import _kernels as K
    n = 64
    W, G, S1, S2 = (torch.ones(n, device=gpu) for _ in range(4))
    Wc = torch.ones(n, device=gpu, dtype=torch.bfloat16)
    step = torch.tensor([STEP], device=gpu)
    if bad == "dtype":
        G = G.double()
    elif bad == "short_state":
        S1 = S1[:n - 4]
    elif bad == "cpu_step":
        step = step.cpu()
    else:
        Wc = Wc[:n - 4]
    with pytest.raises(RuntimeError, match=entry):
        if entry == "sgd":
            K.sgd_update(W, G, S1, Wc, step, 0.0, 0.9, False, zero_grad=True)
        elif entry == "sgd_segs":
            K.C().sgd_segs(W, G, S1, Wc, step, [0], [n], 0.0, 0.9, False, True)
        elif entry == "adam":
            K.adam_update(W, G, S2, S1, Wc, step, 0.9, 0.999, 0.0, EPS, zero_grad=True)
        else:
            K.adagrad_update(W, G, S1, Wc, step, 0.0, 1e-10, zero_grad=True)
    torch.cuda.synchronize()
    for t in (W, G, S1, S2, Wc):
        assert int((t != 1).sum()) == 0
