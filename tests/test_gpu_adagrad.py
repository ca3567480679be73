"""Adagrad on MI355X against float64 torch oracles: the dense update kernel
(csrc/kernels/optim.hip fm_adagrad_update), the fused sparse table update (csrc/kernels/embedding.hip
fm_sdp_coalesce + fm_emb_adagrad_apply: duplicates summed BEFORE the gradient is squared) and a tiny
DLRM trained on HIP (eager and hipGraph-captured) against the CPU executor.

The update is sign-like at H = 0 (g / (|g| + eps) is ill-conditioned near g = 0) and the coalesce
sums duplicates in atomic order, so every comparison with duplicate rows starts from H >= 0.1:
d(update)/dg <= lr / sqrt(0.1), and the bounds follow from the coalesce tolerance of
tests/test_gpu_sparse_dp.py (rtol 1e-5, atol 1e-5 * max(1, sqrt(dup)))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-10


# ------------------------------------------------------------------ dense kernel
@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n,off", [(1031, 1), (1033, 1), (1031, 0)])
def test_dense_update_unaligned_views(gpu, n, off, wd, mirror, zero_grad):
    """An odd n from a view one element into its buffer: scalar head (3 elements), 16-B body and
    (n = 1033) a scalar tail of 2; the aligned view of 1031 has no head and a tail of 3."""
    from flexmi.ops import _kernels as K
    torch.manual_seed(0)

    def view(t):
        return t[off:n + off]
    Wb = torch.randn(n + 2, device=gpu)
    Gb = torch.randn(n + 2, device=gpu)
    Hb = torch.rand(n + 2, device=gpu) * 0.9 + 0.1
    Cb = torch.full((n + 2,), 7.0, device=gpu, dtype=torch.bfloat16)
    edges = [(b[:off].tolist(), b[n + off:].tolist()) for b in (Wb, Gb, Hb, Cb)]
    W, G, H, Wc = view(Wb), view(Gb), view(Hb), (view(Cb) if mirror else None)
    lr = torch.tensor([LR], device=gpu)
    lr64 = float(lr.item())
    w, h = W.double().clone(), H.double().clone()
    for step in range(2):
        if step:
            G.copy_(torch.randn(n, device=gpu))
        g_in = G.clone()
        g = g_in.double() + wd * w
        h += g * g
        w -= lr64 * g / (h.sqrt() + EPS)
        K.adagrad_update(W, G, H, Wc, lr, wd, EPS, zero_grad=zero_grad)
        torch.cuda.synchronize()
        torch.testing.assert_close(W.double(), w, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(H.double(), h, rtol=1e-5, atol=1e-6)
        if zero_grad:
            assert int((G != 0).sum().item()) == 0
        else:
            assert torch.equal(G, g_in)
        if mirror:
            assert torch.equal(Wc, W.bfloat16())
    # nothing outside the views was written
    assert edges == [(b[:off].tolist(), b[n + off:].tolist()) for b in (Wb, Gb, Hb, Cb)]
    if not mirror:
        assert int((Cb != 7.0).sum().item()) == 0


# ------------------------------------------------------------------ sparse coalesce + apply
def _oracle(idx, dy, rows, lo, scale):
    """float64: the lookups of the shard's rows, duplicates summed -> (unique local rows, sums)."""
    B, bag = idx.shape
    li = idx.long().reshape(-1) - lo
    ok = (li >= 0) & (li < rows)
    g = (dy.double() * scale).repeat_interleave(bag, 0)[ok]
    uniq, inv = torch.unique(li[ok], return_inverse=True)
    s = torch.zeros(uniq.numel(), dy.shape[1], dtype=torch.float64, device=dy.device).index_add_(0, inv, g)
    return uniq, s


# (rows held, D, bag, first row, index width): mostly unique rows; ~340 duplicates per row; duplicates
# inside a bag (scale 0.5); a row shard that sees out-of-shard lookups; D % 4 != 0 (scalar fallback)
SPECS = [(50000, 128, 1, 0, torch.int64), (3, 64, 1, 0, torch.int32), (700, 32, 2, 0, torch.int64),
         (400, 128, 1, 300, torch.int64), (97, 6, 1, 0, torch.int64)]


@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
def test_sparse_coalesce_and_apply(gpu, dy_dtype):
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(0)
    B = 1024
    W, H, slot, cid, ids, g, cnt, lo, scale = [], [], [], [], [], [], [], [], []
    for rows, D, bag, l0, it in SPECS:
        W.append(torch.randn(rows, D, device=dev))
        H.append(torch.rand(rows, D, device=dev) * 0.9 + 0.1)
        slot.append(torch.full((rows,), -1, dtype=torch.int32, device=dev))
        cid.append(torch.empty(B * bag, dtype=torch.int32, device=dev))
        ids.append(torch.zeros(B * bag, dtype=torch.int32, device=dev))
        g.append(torch.zeros(B * bag * D, dtype=torch.float32, device=dev))
        cnt.append(torch.zeros(1, dtype=torch.int32, device=dev))
        lo.append(l0)
        scale.append(0.5 if bag == 2 else 1.0)
    lr = torch.tensor([LR], device=dev)
    lr64 = float(lr.item())
    w64 = [w.double().clone() for w in W]
    h64 = [h.double().clone() for h in H]
    for step in range(2):
        idx, dy = [], []
        for rows, D, bag, l0, it in SPECS:
            hi = rows + l0 + (200 if l0 else 0)
            idx.append(torch.randint(0, hi, (B, bag), device=dev, dtype=it))
            dy.append(torch.randn(B, D, device=dev).to(dy_dtype))
        w_before = [w.clone() for w in W]
        h_before = [h.clone() for h in H]
        K.C().sdp_coalesce(W, idx, dy, [d.stride(0) for d in dy], scale, lo, slot, cid, ids, g, cnt)
        K.C().emb_adagrad_apply(W, H, ids, g, cnt, slot, lr, EPS)
        torch.cuda.synchronize()
        for k, (rows, D, bag, l0, _) in enumerate(SPECS):
            uniq, s = _oracle(idx[k], dy[k], rows, l0, scale[k])
            assert 0 < uniq.numel() <= rows
            h64[k][uniq] += s * s
            w64[k][uniq] -= lr64 * s / (h64[k][uniq].sqrt() + EPS)
            dup = max(1.0, (B * bag / uniq.numel()) ** 0.5)
            gmax = float(s.abs().max())
            w_err = float((W[k].double() - w64[k]).abs().max())
            h_rel = float(((H[k].double() - h64[k]).abs() / h64[k]).max())
            print(f"step {step} table {k} rows {rows} D {D} uniq {uniq.numel()}: |dW| {w_err:.3e} rel dH {h_rel:.3e}")
            torch.testing.assert_close(W[k].double(), w64[k], rtol=1e-5, atol=1e-6 + (LR / 0.1 ** 0.5) * 1e-5 * dup)
            torch.testing.assert_close(H[k].double(), h64[k], rtol=2e-5, atol=2e-5 * dup * gmax)
            untouched = torch.ones(rows, dtype=torch.bool, device=dev)
            untouched[uniq] = False
            assert torch.equal(W[k][untouched], w_before[k][untouched])
            assert torch.equal(H[k][untouched], h_before[k][untouched])
            assert int((slot[k] != -1).sum().item()) == 0, "claim slots not released"
            assert int(cnt[k].item()) == 0, "count not reset for the next step"


def test_zero_accumulator_unique_rows(gpu):
    """From H = 0 the first step is lr * g / (|g| + eps): a permutation, so no row repeats."""
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(1)
    rows, D = 512, 128
    W = torch.randn(rows, D, device=dev)
    H = torch.zeros(rows, D, device=dev)
    idx = torch.randperm(rows, device=dev).view(rows, 1)
    dy = torch.randn(rows, D, device=dev)
    slot = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    cid = torch.empty(rows, dtype=torch.int32, device=dev)
    ids = torch.zeros(rows, dtype=torch.int32, device=dev)
    g = torch.zeros(rows * D, dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    lr = torch.tensor([LR], device=dev)
    w0 = W.double().clone()
    K.C().sdp_coalesce([W], [idx], [dy], [D], [1.0], [0], [slot], [cid], [ids], [g], [cnt])
    K.C().emb_adagrad_apply([W], [H], [ids], [g], [cnt], [slot], lr, EPS)
    torch.cuda.synchronize()
    gr = torch.zeros(rows, D, dtype=torch.float64, device=dev)
    gr[idx.view(-1)] = dy.double()
    exp = w0 - float(lr.item()) * gr / (gr.abs() + EPS)
    torch.testing.assert_close(W.double(), exp, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(H.double(), gr * gr, rtol=1e-5, atol=1e-6)
    assert int((slot != -1).sum().item()) == 0 and int(cnt.item()) == 0


def test_apply_rejects_mismatched_buffers(gpu):
    from flexmi.ops import _kernels as K
    dev = gpu
    W = torch.zeros(8, 4, device=dev)
    ids = torch.zeros(16, dtype=torch.int32, device=dev)
    g = torch.zeros(16 * 4, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    slot = torch.full((8,), -1, dtype=torch.int32, device=dev)
    lr = torch.tensor([LR], device=dev)
    with pytest.raises(RuntimeError):     # H of another shape
        K.C().emb_adagrad_apply([W], [torch.zeros(8, 8, device=dev)], [ids], [g], [cnt], [slot], lr, EPS)
    with pytest.raises(RuntimeError):     # payload shorter than ids x D
        K.C().emb_adagrad_apply([W], [torch.zeros(8, 4, device=dev)], [ids], [g[:8]], [cnt], [slot], lr, EPS)
    with pytest.raises(RuntimeError):     # fewer slots than rows
        K.C().emb_adagrad_apply([W], [torch.zeros(8, 4, device=dev)], [ids], [g], [cnt], [slot[:4]], lr, EPS)


@pytest.mark.parametrize("rule", ["adagrad", "rowwise"])
def test_more_tables_than_one_launch_holds(gpu, rule):
    """33 tables: the launchers batch 32 per launch, so the last table runs in a second batch of one
    (its own descriptor set, apply launch and count-zeroing launch).  D alternates 4 (16-B form) and
    6 (scalar form); every table sees a duplicate row across bags and one inside a bag."""
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(2)
    T, rows, B, bag = 33, 8, 4, 2
    Ds = [4 if k % 2 == 0 else 6 for k in range(T)]
    W = [torch.randn(rows, D, device=dev) for D in Ds]
    H = [torch.rand(rows, D if rule == "adagrad" else 1, device=dev) * 0.9 + 0.1 for D in Ds]
    slot = [torch.full((rows,), -1, dtype=torch.int32, device=dev) for _ in Ds]
    cid = [torch.empty(B * bag, dtype=torch.int32, device=dev) for _ in Ds]
    ids = [torch.zeros(B * bag, dtype=torch.int32, device=dev) for _ in Ds]
    g = [torch.zeros(B * bag * D, dtype=torch.float32, device=dev) for D in Ds]
    cnt = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in Ds]
    idx = [torch.tensor([[0, 1], [1, 2], [3, 3], [k % rows, 5]], device=dev) for k in range(T)]
    dy = [torch.randn(B, D, device=dev) for D in Ds]
    lr = torch.tensor([LR], device=dev)
    lr64 = float(lr.item())
    w64 = [w.double().clone() for w in W]
    h64 = [h.double().clone() for h in H]
    w_before = [w.clone() for w in W]
    h_before = [h.clone() for h in H]
    K.C().sdp_coalesce(W, idx, dy, [d.stride(0) for d in dy], [0.5] * T, [0] * T, slot, cid, ids, g, cnt)
    apply = K.C().emb_adagrad_apply if rule == "adagrad" else K.C().emb_rowwise_adagrad_apply
    apply(W, H, ids, g, cnt, slot, lr, EPS)
    torch.cuda.synchronize()
    for k in range(T):
        uniq, s = _oracle(idx[k], dy[k], rows, 0, 0.5)
        assert 0 < uniq.numel() < B * bag
        if rule == "adagrad":
            h64[k][uniq] += s * s
            w64[k][uniq] -= lr64 * s / (h64[k][uniq].sqrt() + EPS)
        else:
            h64[k][uniq] += (s * s).sum(1, keepdim=True) / Ds[k]
            w64[k][uniq] -= lr64 * s / (h64[k][uniq].sqrt() + EPS)
        dup = max(1.0, (B * bag / uniq.numel()) ** 0.5)
        gmax = float(s.abs().max())
        torch.testing.assert_close(W[k].double(), w64[k], rtol=1e-5, atol=1e-6 + (LR / 0.1 ** 0.5) * 1e-5 * dup)
        torch.testing.assert_close(H[k].double(), h64[k], rtol=2e-5, atol=2e-5 * dup * gmax)
        untouched = torch.ones(rows, dtype=torch.bool, device=dev)
        untouched[uniq] = False
        assert torch.equal(W[k][untouched], w_before[k][untouched])
        assert torch.equal(H[k][untouched], h_before[k][untouched])
        assert int(cnt[k].item()) == 0, f"table {k}: count not reset"
        assert int((slot[k] != -1).sum().item()) == 0, f"table {k}: claim slots not released"


# ------------------------------------------------------------------ model level
B_MODEL = 128


def _dlrm_run(dev, use_graph=False):
    from flexmi.core import AdagradOptimizer, FFConfig, FFModel, LossType, MetricsType
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    rng = np.random.RandomState(1)
    dcfg = DLRMConfig.preset("tiny")
    dense = rng.rand(B_MODEL, 13).astype(np.float32)
    sp = [rng.randint(0, r, (B_MODEL, 1)).astype(np.int64) for r in dcfg.embedding_size]
    lab = rng.randint(0, 2, (B_MODEL, 1)).astype(np.float32)
    cfg = FFConfig()
    cfg.batchSize, cfg.device, cfg.compute_dtype = B_MODEL, dev, "fp32"
    m = FFModel(cfg)
    d, s, p = build_dlrm(m, dcfg)
    m.compile(AdagradOptimizer(m, lr=0.05, initial_accumulator_value=0.1), LossType.LOSS_BINARY_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    tables = [ex.wentries[op.weights[0].guid] for op in m.layers if op.op_type == OperatorType.OP_EMBEDDING]
    assert len(tables) == len(dcfg.embedding_size)
    for e in tables:
        assert e.sparse and e.grad is None and set(e.state) == {"h"} and tuple(e.state["h"].shape) == tuple(e.shape)
    dd = np.zeros((B_MODEL, d.dims[1]), np.float32)
    dd[:, :13] = dense
    ex.scatter_from_host(d, dd)
    for t, a in zip(s, sp):
        ex.scatter_from_host(t, a)
    ex.scatter_from_host(m.get_label_tensor(), lab)
    if use_graph:
        ex.train_step()
        run = ex.capture_step()
        for _ in range(2):
            run()
        torch.cuda.synchronize()
    else:
        for _ in range(3):
            ex.train_step()
    ws = [w.get_weights(m) for w in m.parameters]
    ws[0] = ws[0][:, :13]   # drop the (unused, zero-input) padding columns of the first layer
    hs = [e.state["h"].detach().cpu().numpy() for e in tables]
    return ws, m.get_perf_metrics().get_loss(), hs, sp


@pytest.fixture(scope="module")
def cpu_dlrm():
    return _dlrm_run("cpu")


@pytest.mark.parametrize("use_graph", [False, True])
def test_dlrm_tiny_adagrad_gpu_matches_cpu(gpu, cpu_dlrm, use_graph):
    ws, loss, hs, sp = _dlrm_run("gpu", use_graph)
    for a, b in zip(cpu_dlrm[0], ws):
        assert np.abs(a - b).max() < 3e-2 * max(1.0, np.abs(a).max()), (a.shape,)
    assert abs(cpu_dlrm[1] - loss) < 2e-2
    for h, idx in zip(hs, sp):
        untouched = np.ones(h.shape[0], bool)
        untouched[idx.reshape(-1)] = False
        assert h.min() >= np.float32(0.1) and h[~untouched].max() > np.float32(0.1)   # the accumulators moved
        assert np.all(h[untouched] == np.float32(0.1))                                # ... on looked-up rows only
