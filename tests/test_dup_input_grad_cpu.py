"""One tensor at two inputs of one op: ``multiply(a, a)``, ``add(a, a)``, ``subtract(a, a)`` and the
residual form ``relu(add(a, a))``.  Both input gradients land in ``a``'s gradient buffer, so the second
slot has to add to the first; an executor that builds the accumulate flags of an op before it marks
any of that op's inputs written stores twice and trains the layers below on half the gradient.

Model: dense(20 -> 16) -> op(a, a) -> dense(5) -> softmax, sparse categorical cross-entropy, one SGD
step from weights the test sets.  Oracle: the same model in torch autograd, fp64.

Bound.  Per parameter tensor ``|got - expected| <= 2^-10 * max|step| + 2^-22 * max|w|``: the fp32
forward and backward are chains of dot products of at most 20 terms (64 over the batch), each good to
a few 2^-24 relative, far below 2^-10 of the step; the second term is the rounding of the updated
fp32 weight itself.  The lost gradient moves the first layer by half its step, 500 times the bound.
Other ops with several data inputs are refused by ``compile()`` (checked here by name)."""
import numpy as np
import pytest
import torch

B, IN, HID, OUT, LR = 64, 20, 16, 5, 0.5
FORMS = ["multiply", "add", "subtract", "relu_add"]


def _data():
    rng = np.random.RandomState(7)
    x = rng.randn(B, IN).astype(np.float32)
    lab = rng.randint(0, OUT, (B, 1)).astype(np.int32)
    return rng, x, lab


def _torch_step(form, x, lab, ws):
    """One SGD step in fp64; ws are the project's arrays (weights [out, in] or [in, out])."""
    ps = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    w1, b1, w2, b2 = ps

    def lin(v, w, b, nin):
        return v @ (w.t() if w.shape[1] == nin and w.shape[0] != nin else w) + b

    a = lin(torch.tensor(x, dtype=torch.float64), w1, b1, IN)
    h = {"multiply": a * a, "add": a + a, "subtract": a - a, "relu_add": torch.relu(a + a)}[form]
    z = lin(h, w2, b2, HID)
    loss = torch.nn.functional.cross_entropy(z, torch.tensor(lab[:, 0]).long())      # mean over the batch
    loss.backward()
    return [(p - LR * p.grad).detach().numpy() for p in ps], [(LR * p.grad).abs().max().item() for p in ps]


def run_dup_case(form, device, compute_dtype="fp32"):
    """Returns (weights after one step, fp64 expectation, max |step| per tensor, weights before)."""
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    rng, x, lab = _data()
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.seed = B, device, 3
    cfg.compute_dtype = compute_dtype
    m = FFModel(cfg)
    t = m.create_tensor((B, IN))
    a = m.dense(t, HID)
    if form == "relu_add":
        h = m.relu(m.add(a, a))
    else:
        h = getattr(m, form)(a, a)
    m.softmax(m.dense(h, OUT))
    m.compile(SGDOptimizer(m, LR), LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    assert len(m.parameters) == 4
    ws = []
    for p in m.parameters:                      # w1, b1, w2, b2
        w = (0.3 * rng.randn(*p.dims)).astype(np.float32)
        p.set_weights(m, w)
        ws.append(w)
    assert ws[0].size == IN * HID and ws[1].size == HID and ws[2].size == HID * OUT and ws[3].size == OUT
    ex.scatter_from_host(t, x)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    ex.train_step()
    got = [p.get_weights(m) for p in m.parameters]
    exp, step = _torch_step(form, x, lab, ws)
    return got, exp, step, ws


def check_dup_case(form, device):
    got, exp, step, ws = run_dup_case(form, device)
    for i, (g, e, s, w) in enumerate(zip(got, exp, step, ws)):
        err = np.abs(g.astype(np.float64) - e).max()
        bound = 2.0 ** -10 * s + 2.0 ** -22 * np.abs(w).max()
        print(f"{form} {device} param {i}: max|got-exp| {err:.3e}  max|step| {s:.3e}  bound {bound:.3e}")
        assert err <= bound, (form, i, err, s, bound)
    if form == "subtract":
        # a - a is 0 whatever a is: nothing reaches the first layer, the second bias still learns
        assert np.array_equal(got[0], ws[0]) and np.array_equal(got[1], ws[1])
        assert step[3] > 1e-3 and np.abs(got[3] - ws[3]).max() > 0.5 * step[3]
    else:
        assert step[0] > 1e-3 and step[1] > 1e-3        # the case can tell half a gradient from a whole one


@pytest.mark.parametrize("form", FORMS)
def test_dup_input_grad_cpu(form):
    check_dup_case(form, "cpu")


@pytest.mark.parametrize("opname", ["concat", "batch_matmul"])
def test_other_ops_refuse_duplicate_inputs(opname):
    from flexmi.core import FFConfig, FFModel, LossType, SGDOptimizer
    cfg = FFConfig()
    cfg.batchSize, cfg.device = 8, "cpu"
    m = FFModel(cfg)
    if opname == "concat":
        a = m.dense(m.create_tensor((8, 6)), 4)
        m.dense(m.concat([a, a], 1), 3)
    else:
        a = m.dense(m.create_tensor((8, 4, 4)), 4)
        m.flat(m.batch_matmul(a, a))
    with pytest.raises(ValueError, match="Concat|BatchMatmul"):
        m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
