"""METRICS_AUC on the GPU: fm_auc_hist (csrc/kernels/auc.hip) against the torch oracle, integer for
integer, and the executor state in eager and hipGraph-replayed steps."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPECIAL = [-math.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, math.inf]


def logistic_set(n, seed=0):
    """y ~ Bernoulli(0.25), z ~ N(0, 1.5) + y - 2, p = sigmoid(z) as fp32; both classes present."""
    rng = np.random.RandomState(seed)
    y = rng.rand(n) < 0.25
    y[0], y[1 % n] = True, False
    z = rng.normal(0.0, 1.5, n) + y - 2.0
    p = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    return torch.from_numpy(p), torch.from_numpy(y.astype(np.float32))


def exact_auc(scores, labels):
    """Rank-statistic AUC with ties counted 1/2, as a Fraction."""
    groups = {}
    for s, y in zip(scores.float().reshape(-1).tolist(), labels.float().reshape(-1).tolist()):
        groups.setdefault(s, [0, 0])[1 if y >= 0.5 else 0] += 1
    below, num, P, N = 0, 0, 0, 0
    for s in sorted(groups):
        n, p = groups[s]
        num += p * (2 * below + n)
        below += n
        P += p
        N += n
    return Fraction(num, 2 * P * N)


def _score_sets(n, seed):
    p, y = logistic_set(n, seed)
    alt = torch.arange(n) % 2
    # two values, labels alternating with another period: each value meets both classes, so the
    # peel loop must separate the classes inside one bin
    two = torch.where(alt == 0, torch.tensor(0.25), torch.tensor(0.75))
    sp = torch.tensor(SPECIAL + [math.nan], dtype=torch.float32).repeat(n // 9 + 1)[:n]
    return {
        "logistic": (p, y),
        "all_equal": (torch.full((n,), 0.5), (torch.arange(n) % 3 == 0).float()),
        "two_values": (two, ((torch.arange(n) + seed) % 3 != 0).float()),
        "special": (sp, ((torch.arange(n) + seed) % 2).float()),
    }


@pytest.fixture(scope="module")
def state(gpu):
    from flexmi.core.loss_metrics import AUC_BINS
    return torch.zeros(2, AUC_BINS, dtype=torch.int64, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4133])
def test_kernel_equals_oracle(gpu, state, n, dtype):
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT, auc_hist_torch
    from flexmi.ops import _kernels as K
    hist, inv = state
    first, second = _score_sets(n, 0), _score_sets(n, 1)
    for name in first:
        hist.zero_()
        inv.zero_()
        want = torch.zeros(2, AUC_BINS, dtype=torch.int64)
        winv = torch.zeros(1, dtype=torch.int64)
        for s, y in (first[name], second[name]):          # two accumulating calls
            s = s.to(dtype)
            auc_hist_torch(s, y, want, winv, AUC_SHIFT)
            K.auc_hist(s.to(gpu).reshape(n, 1), y.to(gpu).reshape(n, 1), hist, inv, AUC_SHIFT)
        got, ginv = hist.cpu(), int(inv.cpu())
        assert int(got.sum()) + ginv == 2 * n, name
        assert ginv == int(winv), name
        assert torch.equal(got, want), (name, (got != want).nonzero()[:8].tolist())
        if name == "special" and n >= 9:
            assert ginv > 0
    # B = 0 leaves the state untouched
    before = hist.clone()
    K.auc_hist(torch.empty(0, 1, dtype=dtype, device=gpu), torch.empty(0, 1, device=gpu), hist, inv, AUC_SHIFT)
    torch.cuda.synchronize()
    assert torch.equal(hist, before) and int(inv.cpu()) == ginv


@pytest.mark.parametrize("rounds", [0, 1, 64])
def test_kernel_peel_rounds_do_not_change_the_counts(gpu, state, rounds):
    """The shipped kernel folds equal keys per wave until a few rounds found a lone key, then lets
    the other lanes add 1 each; one atomic per sample (0), giving up at the first lone key (1) and
    the full peel (64) count the same."""
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT, auc_hist_torch
    from flexmi.ops import _kernels as K
    hist, inv = state
    n = 4133
    for name, (s, y) in _score_sets(n, 2).items():
        hist.zero_()
        inv.zero_()
        want = torch.zeros(2, AUC_BINS, dtype=torch.int64)
        winv = torch.zeros(1, dtype=torch.int64)
        auc_hist_torch(s, y, want, winv, AUC_SHIFT)
        K.auc_hist(s.to(gpu).reshape(n, 1), y.to(gpu).reshape(n, 1), hist, inv, AUC_SHIFT, rounds=rounds)
        assert torch.equal(hist.cpu(), want) and int(inv.cpu()) == int(winv), name


def _tiny(batch, lr):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    cfg = FFConfig()
    cfg.batchSize = batch
    m = FFModel(cfg)
    d, s, _ = build_dlrm(m, DLRMConfig.preset("tiny"))
    m.compile(SGDOptimizer(m, lr), LossType.LOSS_BINARY_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY, MetricsType.METRICS_AUC])
    return m, d, s


def _feed(m, d, s, it, batch):
    from flexmi.models.dlrm import DLRMConfig
    ex = m._ex()
    rng = np.random.RandomState(100 + it)
    dd = np.zeros((batch, d.dims[1]), np.float32)
    dd[:, :13] = rng.rand(batch, 13)
    ex.scatter_from_host(d, dd)
    for t, r in zip(s, DLRMConfig.preset("tiny").embedding_size):
        ex.scatter_from_host(t, rng.randint(0, r, (batch, 1)).astype(np.int64))
    lab = (rng.rand(batch, 1) < 0.3).astype(np.float32)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    return lab


def test_model_eager_histogram_equals_oracle(gpu):
    from flexmi.core.loss_metrics import AUC_BINS, AUC_SHIFT, auc_hist_torch
    batch = 256
    m, d, s = _tiny(batch, 0.05)
    ex = m.init_layers()
    assert ex.backend == "hip" and ex.auc_hist.is_cuda
    ex.training = False
    m.reset_metrics()
    preds, labs = [], []
    for it in range(3):
        labs.append(_feed(m, d, s, it, batch))
        m.forward()
        m.compute_metrics()
        preds.append(ex.gather_to_host(m.get_output_tensor()).copy())
    p, y = torch.from_numpy(np.concatenate(preds)), torch.from_numpy(np.concatenate(labs))
    want = torch.zeros(2, AUC_BINS, dtype=torch.int64)
    winv = torch.zeros(1, dtype=torch.int64)
    auc_hist_torch(p, y, want, winv, AUC_SHIFT)
    assert torch.equal(ex.auc_hist.cpu(), want) and int(ex.auc_invalid.cpu()) == 0
    pm = m.get_perf_metrics()
    assert pm.auc_pos + pm.auc_neg == 3 * batch and pm.auc_pos == int(y.sum())
    exact = exact_auc(p, y)
    print(f"auc={pm.get_auc()!r} exact={float(exact)!r} bound={pm.get_auc_bound():.3e} dtype={ex.logits_buf.dtype}")
    assert abs(Fraction(pm.get_auc()) - exact) <= Fraction(pm.get_auc_bound()) + Fraction(1e-12)
    if ex.logits_buf.dtype == torch.bfloat16:
        assert abs(Fraction(pm.get_auc()) - exact) <= Fraction(1e-12)


def test_model_captured_steps_accumulate(gpu):
    batch = 256
    m, d, s = _tiny(batch, 0.0)           # lr 0: every replay sees the same weights
    ex = m.init_layers()
    _feed(m, d, s, 0, batch)
    m.reset_metrics()
    m.forward()
    m.compute_metrics()
    single = ex.auc_hist.clone()
    assert int(single.sum()) == batch
    m.reset_metrics()
    for _ in range(5):                    # eager, captured, then three hipGraph replays
        m.begin_trace(111)
        m.forward()
        m.zero_gradients()
        m.backward()
        m.update()
        m.end_trace(111)
    torch.cuda.synchronize()
    assert m._traces[111]["replay"] is not None, "the step was not captured"
    assert torch.equal(ex.auc_hist, 5 * single)
    pm = m.get_perf_metrics()
    assert pm.auc_pos + pm.auc_neg == 5 * batch and pm.auc_invalid == 0
