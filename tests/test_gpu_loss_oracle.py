"""The fused loss + metrics kernels (csrc/kernels/loss.hip: fm_loss_kernel, a wave per row, and
fm_loss1_kernel, a thread per row when C == 1) against an fp64 re-statement of
``flexmi.core.loss_metrics.loss_and_metrics_torch``: all eight slots and the gradient, the
--loss-threshold clamp, and the metrics mask as the reference applies it (slots 1-6 only under their
bit; slot 3 is -log p[argmax y] for any label form).  ``test_oracle_matches_reference_cpu`` holds the
oracle to the project's fp32 reference on the CPU, so it cannot drift from it.

Bounds:
  * slots 0 and 1 are integers below 2^24: exact.
  * fp32 gradient: |got - ref| <= 2^-22 |scale| (|p| + |y|) per element: the subtraction and the
    multiply round once each, 2 * 2^-24 of at most |scale| (|p| + |y|), with a margin of two.
  * bf16 gradient: one more rounding, to bf16: 2^-8 |ref| on top of the fp32 bound.
  * slots 2-7, relative to the sum of the magnitudes of their terms: 2^-16 at B = 777 (at most 195
    blocks of sequential fp32 atomics at 2^-24 each, plus a few ulp per term from __logf; one missing
    row moves a sum by 1.3e-3), 2^-13 in the striding cases (up to 2048 blocks).
Sparse categorical cross-entropy needs C >= 2 (one class leaves nothing to label)."""
import numpy as np
import pytest
import torch

from flexmi.core.loss_metrics import loss_and_metrics_torch
from flexmi.ops import _kernels as Kk

gpu_test = pytest.mark.gpu

CCE, SCCE, MSE_AVG, MSE_SUM, BCE = 50, 51, 52, 53, 54
F32 = lambda v: float(np.float32(v))        # noqa: E731  a constant as an fp32 kernel / tensor op sees it
LOG_MIN = F32(1e-7)
LOG_MAX = F32(1 - 1e-7)
CASES = [(lt, C) for lt in (CCE, SCCE, MSE_AVG, MSE_SUM, BCE) for C in (1, 2, 7, 64, 65, 130)
         if not (lt == SCCE and C == 1)]


def _first_argmax(v):
    C = v.shape[1]
    idx = torch.arange(C).expand_as(v)
    return torch.where(v == v.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def oracle(loss_type, logits, labels, scale, mask, clamp=0.0):
    """fp64 restatement of loss_and_metrics_torch.  Returns (grad [B, C], slots [8], mags [8]): mags
    is the sum of the magnitudes of the terms of each slot (0 where the mask drops the slot)."""
    B = logits.shape[0]
    p = logits.double().reshape(B, -1)
    C = p.shape[1]
    keep = torch.ones_like(p)
    if clamp > 0.0:
        pc = p.clamp(F32(clamp), F32(1.0 - clamp))
        keep = (pc == p).double()
        p = pc
    if loss_type == SCCE:
        y = torch.zeros_like(p)
        y[torch.arange(B), labels.reshape(B).long()] = 1.0
    else:
        y = labels.double().reshape(B, -1)
    grad = (p - y) * scale * keep
    slots, mags = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)

    def put(s, terms):
        slots[s] += terms.sum()
        mags[s] += terms.abs().sum()

    slots[0] = B
    ay = _first_argmax(y)
    if mask & 1:
        ok = ((p[:, 0] >= 0.5) == (y[:, 0] >= 0.5)) if C == 1 else (_first_argmax(p) == ay)
        slots[1] = ok.sum()
    cce = -(y * torch.log(p.clamp_min(LOG_MIN)))
    d = p - y
    se = (d * d).sum(1)
    if mask & 2:
        put(2, cce)
    if mask & 4:
        put(3, -torch.log(p.gather(1, ay[:, None]).clamp_min(LOG_MIN)))
    if mask & 8:
        put(4, d * d)
    if mask & 16:
        put(5, se.sqrt())
    if mask & 32:
        put(6, d.abs())
    if loss_type == BCE:
        pc = p.clamp(LOG_MIN, LOG_MAX)
        put(7, -(y * torch.log(pc)))
        put(7, -((1 - y) * torch.log(1 - pc)))
    elif loss_type in (CCE, SCCE):
        put(7, cce)
    else:
        put(7, d * d)
    return grad, slots, mags, p, y


def make_case(loss_type, B, C, ldt=torch.float32, clamp=0.0, seed=0):
    """(logits rounded to ldt, labels).  Rows 0-5 hold ties and edge values."""
    g = torch.Generator().manual_seed(1000 * loss_type + 10 * C + seed)
    if C == 1 or loss_type == BCE:
        p = torch.rand(B, C, generator=g)
    else:
        p = torch.softmax(torch.randn(B, C, generator=g), -1)
    if loss_type == SCCE:
        lab = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    elif loss_type == CCE:
        lab = torch.nn.functional.one_hot(torch.randint(0, C, (B,), generator=g), C).float()
    elif loss_type == BCE:
        lab = torch.randint(0, 2, (B, C), generator=g).float()
    else:
        lab = torch.rand(B, C, generator=g)
    if B > 6:
        if C > 1:
            j = 67 if C > 67 else C - 1                 # with C > 64, a tie between two passes of one lane
            p[0, 3 % C] = p[0, j] = 0.75                # tied maxima in p: the first index wins
            p[1, j] = p[1, 3 % C] = 0.75
            if loss_type in (MSE_AVG, MSE_SUM, BCE):
                lab[0, 0] = lab[0, j] = 1.5             # tied maxima in y
                lab[2, j] = lab[2, 0] = 1.5
        p[3, 0] = 0.0                                   # log clamped at LOG_MIN
        p[4, 0] = 1.0                                   # 1 - p clamped for BCE
        if loss_type == SCCE:
            lab[3] = 0
        elif loss_type in (CCE, BCE):
            lab[3] = 0.0
            lab[3, 0] = 1.0
            lab[4, 0] = 0.0
        if clamp > 0.0:
            p[5, 0] = F32(clamp)                        # exactly at the bounds: not clipped
            p[6, 0] = F32(1.0 - clamp)
            p[7:12, 0] = torch.tensor([0.0, clamp / 2, 1.0 - clamp / 2, 1.0, 0.5])
    return p.to(ldt), lab


def grad_bound(gdt, ref, p, y, scale):
    b = 2.0 ** -22 * abs(scale) * (p.abs() + y.abs())
    return b + 2.0 ** -8 * ref.abs() if gdt == torch.bfloat16 else b


def check(acc, grad, ref_grad, slots, mags, p, y, scale, tol, what, calls=1):
    acc = acc.cpu().double()
    assert acc[0].item() == calls * slots[0].item() and acc[1].item() == calls * slots[1].item(), (what, acc, slots)
    for s in range(2, 8):
        err, bound = abs(acc[s].item() - calls * slots[s].item()), tol * calls * mags[s].item()
        assert err <= bound, (what, s, acc[s].item(), slots[s].item(), err, bound)
    if grad is not None:
        got = grad.cpu().double().reshape(ref_grad.shape)
        err, bound = (got - ref_grad).abs(), grad_bound(grad.dtype, ref_grad, p, y, scale)
        assert bool((err <= bound).all()), (what, (err - bound).max().item())


def run_hip(gpu, loss_type, p, lab, gdt, scale, mask, clamp, acc=None):
    B = p.shape[0]
    acc = torch.zeros(8, device=gpu) if acc is None else acc
    grad = None if gdt is None else torch.full(tuple(p.shape), 7.0, dtype=gdt, device=gpu)
    Kk.loss_forward_backward(loss_type, p.to(gpu), lab.to(gpu), grad, scale, acc, mask, clamp)
    return acc, grad


# ---------------------------------------------------------------- the oracle against the reference (CPU)
@pytest.mark.parametrize("loss_type,C", CASES)
def test_oracle_matches_reference_cpu(loss_type, C):
    for clamp in (0.0, 0.1):
        for mask in (63, 1, 0, 2 | 8, 4):
            p, lab = make_case(loss_type, 777, C, clamp=clamp)
            scale = 1.0 / 777
            ref_grad, slots, mags, pc, y = oracle(loss_type, p, lab, scale, mask, clamp)
            grad, acc = torch.empty_like(p), torch.zeros(8)
            loss_and_metrics_torch(loss_type, p, lab, grad, scale, acc, mask, clamp=clamp)
            check(acc, grad, ref_grad, slots, mags, pc, y, scale, 2.0 ** -16, ("cpu", loss_type, C, clamp, mask))
            for s in range(1, 7):
                if not (mask >> (s - 1)) & 1:
                    assert acc[s].item() == 0.0 and slots[s].item() == 0.0


# ---------------------------------------------------------------- B = 777: every loss, C, dtype pairing, clamp
@gpu_test
@pytest.mark.parametrize("loss_type,C", CASES)
def test_loss_precise(gpu, loss_type, C):
    scale = 1.0 / 777
    for ldt in (torch.float32, torch.bfloat16):
        for clamp in (0.0, 0.1):
            p, lab = make_case(loss_type, 777, C, ldt, clamp)
            ref_grad, slots, mags, pc, y = oracle(loss_type, p, lab, scale, 63, clamp)
            for gdt in (torch.float32, torch.bfloat16, None):
                acc, grad = run_hip(gpu, loss_type, p, lab, gdt, scale, 63, clamp)
                check(acc, grad, ref_grad, slots, mags, pc, y, scale, 2.0 ** -16, (loss_type, C, ldt, gdt, clamp))


@gpu_test
@pytest.mark.parametrize("loss_type,C", [(CCE, 7), (CCE, 1), (SCCE, 7), (SCCE, 65), (MSE_AVG, 1), (MSE_SUM, 7), (BCE, 1), (BCE, 2)])
def test_loss_masks_and_accumulation(gpu, loss_type, C):
    """Each mask adds only its slots (one-hot labels under bit 4 among them); a second call into the
    same accumulator adds the same again."""
    scale = 0.25
    p, lab = make_case(loss_type, 777, C)
    for mask in (63, 1, 0, 2 | 8, 4):
        ref_grad, slots, mags, pc, y = oracle(loss_type, p, lab, scale, mask)
        acc, grad = run_hip(gpu, loss_type, p, lab, torch.float32, scale, mask, 0.0)
        check(acc, grad, ref_grad, slots, mags, pc, y, scale, 2.0 ** -16, (loss_type, C, mask))
        for s in range(1, 7):
            if not (mask >> (s - 1)) & 1:
                assert acc[s].item() == 0.0, (loss_type, C, mask, s)
        if mask & 4:
            assert slots[3].item() > 100.0           # -log p[argmax y] is there to be missed
        acc, _ = run_hip(gpu, loss_type, p, lab, None, scale, mask, 0.0, acc=acc)
        check(acc, None, ref_grad, slots, mags, pc, y, scale, 2.0 ** -16, (loss_type, C, mask, "twice"), calls=2)


@gpu_test
@pytest.mark.parametrize("loss_type,C", [(CCE, 7), (SCCE, 130), (MSE_AVG, 1), (BCE, 1), (BCE, 65)])
def test_loss_three_rows(gpu, loss_type, C):
    """B = 3: fewer rows than one block has waves."""
    p, lab = make_case(loss_type, 3, C)
    ref_grad, slots, mags, pc, y = oracle(loss_type, p, lab, 1.0 / 3, 63)
    for gdt in (torch.float32, torch.bfloat16):
        acc, grad = run_hip(gpu, loss_type, p, lab, gdt, 1.0 / 3, 63, 0.0)
        check(acc, grad, ref_grad, slots, mags, pc, y, 1.0 / 3, 2.0 ** -16, (loss_type, C, gdt))


# ---------------------------------------------------------------- past one pass of the grid
@gpu_test
@pytest.mark.parametrize("loss_type,B,C", [(CCE, 4 * 2048 + 3, 3), (SCCE, 4 * 2048 + 3, 3), (MSE_SUM, 4 * 2048 + 3, 3),
                                           (BCE, 1024 * 256 + 5, 1), (MSE_AVG, 1024 * 256 + 5, 1)])
def test_loss_grid_stride(gpu, loss_type, B, C):
    """Body rows predict their label (p within 0.02 of y), so their terms are small; the rows past the
    first pass are wrong by a lot (y = 1 at p = 1e-3).  Dropped or repeated, even one of them moves the
    loss sum by 8 times its 2^-13 bound or more."""
    g = torch.Generator().manual_seed(B + loss_type)
    cls = torch.randint(0, C, (B,), generator=g)
    y = torch.nn.functional.one_hot(cls, C).float() if C > 1 else torch.randint(0, 2, (B, 1), generator=g).float()
    p = 0.01 + 0.98 * y + 0.005 * (torch.rand(B, C, generator=g) - 0.5)
    tail = B - (4 * 2048 if C == 3 else 1024 * 256)
    assert 0 < tail <= 5
    p[-tail:] = 1e-3
    y[-tail:] = 0.0
    y[-tail:, C - 1] = 1.0
    cls[-tail:] = C - 1
    lab = cls.to(torch.int32) if loss_type == SCCE else y
    scale = 1.0 / B
    for ldt, gdt in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
        pl = p.to(ldt)
        ref_grad, slots, mags, pc, yy = oracle(loss_type, pl, lab, scale, 63)
        one_row = float(np.log(1e3)) if loss_type in (CCE, SCCE, BCE) else 0.99
        assert one_row > 8 * 2.0 ** -13 * mags[7].item()
        acc, grad = run_hip(gpu, loss_type, pl, lab, gdt, scale, 63, 0.0)
        check(acc, grad, ref_grad, slots, mags, pc, yy, scale, 2.0 ** -13, (loss_type, B, C, ldt))


# ---------------------------------------------------------------- binding checks (nothing is launched)
@gpu_test
def test_loss_binding_refuses_bad_operands(gpu):
    B, C = 8, 4
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=gpu)      # noqa: E731
    good = dict(logits=z(B, C), labels=z(B, C), grad=z(B, C), acc=z(8))
    Kk.C().loss(MSE_AVG, good["logits"], good["labels"], good["grad"], 1.0, good["acc"], 63, 0.0)     # the form is accepted
    bad = [
        (MSE_AVG, dict(logits=z(B, 2 * C)[:, ::2])),                # non-contiguous logits
        (MSE_AVG, dict(logits=z(B, C, dt=torch.float16))),
        (MSE_AVG, dict(logits=torch.zeros(B, C))),                  # host tensor
        (MSE_AVG, dict(grad=z(B, 2 * C)[:, ::2])),
        (MSE_AVG, dict(grad=z(B, C, dt=torch.float64))),
        (MSE_AVG, dict(grad=z(B, C + 1))),
        (MSE_AVG, dict(labels=z(B, C, dt=torch.bfloat16))),
        (MSE_AVG, dict(labels=z(B, C - 1))),
        (MSE_AVG, dict(labels=z(B, 2 * C)[:, ::2])),
        (SCCE, dict(labels=z(B, dt=torch.int64))),                  # the kernel reads int32
        (SCCE, dict(labels=z(B, C))),
        (SCCE, dict(labels=z(B + 1, dt=torch.int32))),
        (MSE_AVG, dict(acc=z(7))),
        (MSE_AVG, dict(acc=z(8, dt=torch.float64))),
        (MSE_AVG, dict(acc=torch.zeros(8))),
    ]
    for loss_type, change in bad:
        a = dict(good, **change)
        if loss_type == SCCE and "labels" not in change:
            a["labels"] = z(B, dt=torch.int32)
        with pytest.raises(RuntimeError):
            Kk.C().loss(loss_type, a["logits"], a["labels"], a["grad"], 1.0, a["acc"], 63, 0.0)
    Kk.C().loss(SCCE, good["logits"], z(B, dt=torch.int32), None, 1.0, good["acc"], 63, 0.0)


# ---------------------------------------------------------------- the executor's accumulators
def _executor_sums(device):
    """One training step of dense(6 -> 1, sigmoid) under BCE with only accuracy requested: the
    executor's accumulators hold the cce, mse, rmse and mae sums too (PerfMetrics.get_mse() reads them
    unasked), on every backend alike; sparse CCE stays on request."""
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
    from flexmi.core.types import ActiMode
    B = 96
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.seed, cfg.compute_dtype = B, device, 4, "fp32"
    m = FFModel(cfg)
    t = m.create_tensor((B, 6))
    m.dense(t, 1, ActiMode.AC_MODE_SIGMOID)
    m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    rng = np.random.RandomState(2)
    ex.scatter_from_host(t, rng.randn(B, 6).astype(np.float32))
    lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    ex.train_step()
    p = ex.logits_buf.detach().cpu().float().reshape(B, 1)
    _, slots, mags, _, _ = oracle(BCE, p, torch.from_numpy(lab), 1.0 / B, 1 | 2 | 8 | 16 | 32)
    acc = ex.metric_acc.detach().cpu().double()
    assert acc[0].item() == B and acc[1].item() == slots[1].item() and acc[3].item() == 0.0
    for s in (2, 4, 5, 6, 7):
        assert mags[s].item() > 1.0 and abs(acc[s].item() - slots[s].item()) <= 2.0 ** -16 * mags[s].item(), (s, acc, slots)
    assert abs(m.get_perf_metrics().get_mse() - slots[4].item() / B) <= 1e-6


def test_executor_sums_cpu():
    _executor_sums("cpu")


@gpu_test
def test_executor_sums_gpu(gpu):
    _executor_sums("gpu")
