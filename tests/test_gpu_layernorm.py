"""csrc/kernels/layernorm.hip against a float64 oracle in bf16 and fp32, strided operands with guard
bytes, run-to-run determinism, and an encoder model on the GPU (eager and captured) against the CPU."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# max-normalised bounds of tests/test_gpu_attention.py and test_gpu_cross.py; W_TOL: the fp32 weight gradients
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}
BWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
W_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-3}
EPS = 1e-5


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _oracle(x, r, gamma, beta, dy, rms):
    """float64 y, ds, dgamma, dbeta of the given (storage-precision) operands."""
    leaf = lambda t: None if t is None else t.double().clone().requires_grad_()   # noqa: E731
    xs, rs, g, b = leaf(x), leaf(r), leaf(gamma), leaf(beta)
    s = xs if rs is None else xs + rs
    if rms:
        y = s * torch.rsqrt((s * s).mean(-1, keepdim=True) + EPS) * (1 if g is None else g)
    else:
        y = torch.nn.functional.layer_norm(s, s.shape[-1:], g, b, EPS)
    y.backward(dy.double())
    return y.detach(), xs.grad, None if g is None else g.grad, None if b is None else b.grad


def _check(x, r, y, dy, dx, dr, accs, affine, rms, dt):
    """Forward into `y`, backward into `dx` / `dr` (None: absent) and fresh random weight gradients, all against the oracle."""
    from flexmi.ops import _kernels as Kk
    R, D = x.shape
    torch.manual_seed(11)
    gamma = torch.randn(D, device=x.device) if affine else None
    beta = torch.randn(D, device=x.device) if affine and not rms else None
    yref, dsref, dgref, dbref = _oracle(x, r, gamma, beta, dy, rms)
    stats = torch.empty((R,) if rms else (R, 2), device=x.device)
    Kk.layernorm_forward(x, r, y, gamma, beta, stats, EPS, rms)
    dgam, dbet = (None if w is None else torch.randn_like(w) for w in (gamma, beta))
    old = [None if g is None else g.double().clone() for g in (dx, dr, dgam, dbet)]
    Kk.layernorm_backward(x, r, dy, gamma, stats, dx, dr, accs[0], accs[1], dgam, dbet, rms)
    ein = [rel_err(g, dsref + (o if a else 0)) for g, o, a in zip((dx, dr), old, accs) if g is not None]
    ew = [rel_err(g, ref + o) for g, ref, o in zip((dgam, dbet), (dgref, dbref), old[2:]) if g is not None]
    print("rel_err y, dx/dresidual, dgamma/dbeta:", rel_err(y, yref), ein, ew)
    assert rel_err(y, yref) < FWD_TOL[dt] and max(ein + [0]) < BWD_TOL[dt] and max(ew + [0]) < W_TOL[dt]


# (R, D, rms, residual, affine, offset of x, dx present, accumulate dx / dresidual), in order: masked lanes and the
# element path; D no power of two, last wave not full; D % 4 == 0 but not % 8; a group-size step (offset 256: E[s^2] -
# mean^2 fails fp32); the block form at the largest D; a one-trip grid of 257 blocks; weight gradients alone; the row loop
# both ways: 70001 rows (32 a block) and 2100 block-form rows pass the grid caps 2048 (forward), 1024 and 768 (backward).
CASES = [(5, 3, False, False, True, 0, True, (True, False)), (37, 40, False, True, True, 0, True, (False, True)),
         (37, 100, True, True, True, 0, True, (True, True)), (9, 1032, False, False, False, 256, True, (False, False)),
         (3, 8192, False, True, True, 256, True, (True, False)), (4099, 128, False, True, True, 0, True, (False, True)),
         (37, 40, False, False, True, 0, False, (False, False)), (70001, 40, False, True, True, 0, True, (True, False)),
         (2100, 2056, False, True, True, 0, True, (False, True))]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c[:7]))
def test_layernorm_vs_float64(gpu, case, dt):
    (R, D, rms, residual, affine, offset, has_dx, accs), _ = case, torch.manual_seed(7)
    mk = lambda: torch.randn(R, D, device=gpu).to(dt)   # noqa: E731
    x, r = (torch.randn(R, D, device=gpu) + offset).to(dt), (mk() if residual else None)
    dxbuf, dr = mk(), (mk() if residual else None)
    keep = dxbuf.clone()
    _check(x, r, torch.full_like(x, 7.0), mk(), dxbuf if has_dx else None, dr, accs, affine, rms, dt)
    assert has_dx or torch.equal(dxbuf, keep)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_layernorm_strided_and_guards(gpu, dt, shift):
    """x, residual: column slices of one [R, 2D + 8] buffer; the rest: leading columns of sentinel-filled ones; shift: bases off by one."""
    R, D, _ = 37, 40, torch.manual_seed(8)
    flats = []       # the whole buffers, the element before a shifted base included
    wide = lambda w, fill: flats.append((torch.randn(R * w + shift, device=gpu) if fill is None else   # noqa: E731
                                         torch.full((R * w + shift,), fill, device=gpu)).to(dt)) or flats[-1][shift:].view(R, w)
    xr, ybuf, dybuf, dxbuf, drbuf = wide(2 * D + 8, None), wide(D + 8, 7.0), wide(D + 16, 7.0), wide(D + 8, 7.0), wide(D + 24, 7.0)
    for b in (dybuf, dxbuf, drbuf):
        b[:, :D] = torch.randn(R, D, device=gpu).to(dt)
    before = [f.clone() for f in flats]
    _check(xr[:, :D], xr[:, D + 8:], ybuf[:, :D], dybuf[:, :D], dxbuf[:, :D], drbuf[:, :D], (True, False), True, False, dt)
    assert all((b[:, D:] == 7).all() for b in (ybuf, dxbuf, drbuf))           # nothing written past column D
    assert all(torch.equal(a[:shift], b[:shift]) for a, b in zip(before, flats))   # nor before a shifted base
    assert torch.equal(before[0], flats[0]) and torch.equal(before[2], flats[2])   # no input (x and r, dy) touched


@pytest.mark.parametrize("R", [4099, 33000], ids=["one-trip", "looping"])
def test_layernorm_backward_is_deterministic(gpu, R):
    from flexmi.ops import _kernels as Kk
    D, _ = 128, torch.manual_seed(9)
    x, r, dy = (torch.randn(R, D, device=gpu).bfloat16() for _ in range(3))
    gamma, stats = torch.randn(D, device=gpu), torch.empty(R, 2, device=gpu)
    Kk.layernorm_forward(x, r, torch.empty_like(x), gamma, torch.zeros_like(gamma), stats, EPS, False)
    runs = []
    for _ in range(2):
        out = [torch.empty_like(x), torch.zeros_like(gamma), torch.zeros_like(gamma)]
        Kk.layernorm_backward(x, r, dy, gamma, stats, out[0], None, False, False, out[1], out[2], False)
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@functools.lru_cache(maxsize=None)
def _train(dev, graph=False, steps=3, B=16, T=48, E=64, heads=2, ff=128):
    """3 SGD steps of two post-norm encoder layers in fp32, bias-free as in tests/test_gpu_attention.py."""
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype, cfg.seed = B, dev, "fp32", 5
    m = FFModel(cfg)
    x = h = m.create_tensor([B, T, E])
    for i in range(2):
        h = m.transformer_encoder_layer(h, heads, ff, causal=True, name=f"enc{i}", attention_bias=False)
    m.dense(h, 1)
    m.compile(SGDOptimizer(m, 0.002), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    rng = np.random.RandomState(0)

    def feed():
        ex.scatter_from_host(x, rng.randn(*x.dims).astype(np.float32))
        ex.scatter_from_host(m.get_label_tensor(), rng.randn(*x.dims[:2], 1).astype(np.float32))

    feed()
    ex.train_step()
    run = ex.capture_step() if graph else ex.train_step
    for _ in range(1, steps):
        feed()
        run()
    if dev == "gpu":
        torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters], m.get_perf_metrics().get_loss()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_encoder_layer_gpu_matches_cpu(gpu, graph):
    cpu, g = _train("cpu"), _train("gpu", graph)
    for a, b in zip(cpu[0], g[0]):
        assert np.abs(a - b).max() / max(np.abs(a).max(), 1e-6) < 1e-4, a.shape
    assert abs(cpu[1] - g[1]) < 1e-4 * max(1.0, abs(cpu[1]))


def test_layernorm_refused_past_8192(gpu):
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    for dev in ("cpu", "gpu"):
        cfg = FFConfig()
        cfg.batchSize, cfg.device, cfg.compute_dtype = 2, dev, "fp32"
        m = FFModel(cfg)
        m.dense(m.layer_norm(m.create_tensor([2, 8200]), name="wide"), 1)
        if dev == "cpu":
            m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
        else:
            with pytest.raises(ValueError, match="LayerNorm 'wide' .* 8200 .* 8192"):
                m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
