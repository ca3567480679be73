"""Row-wise Adagrad on MI355X against float64 torch oracles: the fused row-wise apply after the
coalesce (csrc/kernels/embedding.hip fm_sdp_coalesce + fm_emb_rowwise_adagrad_apply), the
deterministic merge of gathered replica segments (fm_sdp_rowwise_merge_segments) and a tiny DLRM
trained on HIP (eager and hipGraph-captured) against the CPU executor.

  h[r] += (1/D) sum_c G[r,c]^2;  W[r,c] -= lr G[r,c] / (sqrt(h[r]) + eps),  G = duplicates summed first

Tolerances are those of tests/test_gpu_adagrad.py and their derivation carries over: the same
coalesce (duplicates summed in atomic order: rtol 1e-5, atol 1e-5 * max(1, sqrt(dup)) on G), the
same h >= 0.1 conditioning (d(update)/dG <= lr / sqrt(0.1)), and h a mean of the squares the
element-wise bound already covers.  In the merge test ``dup`` counts the lookups of all replicas."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-10


def _oracle(idx, dy, rows, lo, scale):
    """float64: the lookups of the shard's rows, duplicates summed -> (unique local rows, sums)."""
    B, bag = idx.shape
    li = idx.long().reshape(-1) - lo
    ok = (li >= 0) & (li < rows)
    g = (dy.double() * scale).repeat_interleave(bag, 0)[ok]
    uniq, inv = torch.unique(li[ok], return_inverse=True)
    s = torch.zeros(uniq.numel(), dy.shape[1], dtype=torch.float64, device=dy.device).index_add_(0, inv, g)
    return uniq, s


def _rowwise64(w64, h64, uniq, s, lr64):
    """The rule in float64 on w64 [rows, D] / h64 [rows]."""
    h64[uniq] += (s * s).sum(1) / s.shape[1]
    w64[uniq] -= lr64 * s / (h64[uniq].sqrt() + EPS).unsqueeze(1)


def _check(tag, W, H, w64, h64, uniq, s, lookups, w_before, h_before):
    rows = W.shape[0]
    dup = max(1.0, (lookups / uniq.numel()) ** 0.5)
    gmax = float(s.abs().max())
    w_err = float((W.double() - w64).abs().max())
    h_rel = float(((H.double().view(-1) - h64).abs() / h64).max())
    print(f"{tag} rows {rows} D {W.shape[1]} uniq {uniq.numel()}: |dW| {w_err:.3e} rel dh {h_rel:.3e}")
    torch.testing.assert_close(W.double(), w64, rtol=1e-5, atol=1e-6 + (LR / 0.1 ** 0.5) * 1e-5 * dup)
    torch.testing.assert_close(H.double().view(-1), h64, rtol=2e-5, atol=2e-5 * dup * gmax)
    untouched = torch.ones(rows, dtype=torch.bool, device=W.device)
    untouched[uniq] = False
    assert torch.equal(W[untouched], w_before[untouched])
    assert torch.equal(H[untouched], h_before[untouched])


# (rows held, D, bag, first row, index width): mostly unique rows; ~340 duplicates per row; duplicates
# inside a bag (scale 0.5); a row shard that sees out-of-shard lookups; D % 4 != 0 (scalar form);
# 12 lanes per row (not a power of two); more than one 16-B chunk per lane; one lane per row
SPECS = [(50000, 128, 1, 0, torch.int64), (3, 64, 1, 0, torch.int32), (700, 32, 2, 0, torch.int64),
         (400, 128, 1, 300, torch.int64), (97, 6, 1, 0, torch.int64), (300, 48, 1, 0, torch.int64),
         (200, 512, 1, 0, torch.int32), (64, 4, 1, 0, torch.int64)]


@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
def test_rowwise_coalesce_and_apply(gpu, dy_dtype):
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(0)
    B = 1024
    W, H, slot, cid, ids, g, cnt, lo, scale = [], [], [], [], [], [], [], [], []
    for rows, D, bag, l0, it in SPECS:
        W.append(torch.randn(rows, D, device=dev))
        H.append(torch.rand(rows, 1, device=dev) * 0.9 + 0.1)
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
    h64 = [h.double().view(-1).clone() for h in H]
    for step in range(2):
        idx, dy = [], []
        for rows, D, bag, l0, it in SPECS:
            hi = rows + l0 + (200 if l0 else 0)
            idx.append(torch.randint(0, hi, (B, bag), device=dev, dtype=it))
            dy.append(torch.randn(B, D, device=dev).to(dy_dtype))
        w_before = [w.clone() for w in W]
        h_before = [h.clone() for h in H]
        K.C().sdp_coalesce(W, idx, dy, [d.stride(0) for d in dy], scale, lo, slot, cid, ids, g, cnt)
        K.C().emb_rowwise_adagrad_apply(W, H, ids, g, cnt, slot, lr, EPS)
        torch.cuda.synchronize()
        for k, (rows, D, bag, l0, _) in enumerate(SPECS):
            uniq, s = _oracle(idx[k], dy[k], rows, l0, scale[k])
            assert 0 < uniq.numel() <= rows
            _rowwise64(w64[k], h64[k], uniq, s, lr64)
            _check(f"step {step} table {k}", W[k], H[k], w64[k], h64[k], uniq, s, B * bag, w_before[k], h_before[k])
            assert int((slot[k] != -1).sum().item()) == 0, "claim slots not released"
            assert int(cnt[k].item()) == 0, "count not reset for the next step"


def test_zero_accumulator_unique_rows(gpu):
    """From h = 0 the first step has the closed form h = mean(g^2), W -= lr g / (sqrt(h) + eps): a
    permutation, so no row repeats."""
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(1)
    rows, D = 512, 128
    W = torch.randn(rows, D, device=dev)
    H = torch.zeros(rows, 1, device=dev)
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
    K.C().emb_rowwise_adagrad_apply([W], [H], [ids], [g], [cnt], [slot], lr, EPS)
    torch.cuda.synchronize()
    gr = torch.zeros(rows, D, dtype=torch.float64, device=dev)
    gr[idx.view(-1)] = dy.double()
    h = (gr * gr).mean(1, keepdim=True)
    exp = w0 - float(lr.item()) * gr / (h.sqrt() + EPS)
    torch.testing.assert_close(W.double(), exp, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(H.double(), h, rtol=1e-5, atol=1e-6)
    assert int((slot != -1).sum().item()) == 0 and int(cnt.item()) == 0


# ------------------------------------------------------------------ merge of replica segments
MERGE_SPECS = [(5000, 128), (3, 64), (300, 48), (97, 6)]
R, B_REP = 3, 256


def test_merge_is_deterministic_and_sums_before_squaring(gpu):
    """Three replicas' payloads, gathered; the replica procedure (release own claims, merge in rank
    order, apply) run as replica 0 and as replica 2 gives bit-identical W and h, equal to the
    float64 rule on the segments' SUM."""
    from flexmi.ops import _kernels as K
    dev = gpu
    torch.manual_seed(3)
    n = len(MERGE_SPECS)
    lr = torch.tensor([LR], device=dev)
    lr64 = float(lr.item())
    W0 = [torch.randn(rows, D, device=dev) for rows, D in MERGE_SPECS]
    H0 = [torch.rand(rows, 1, device=dev) * 0.9 + 0.1 for rows, _ in MERGE_SPECS]
    Ds = [D for _, D in MERGE_SPECS]
    # one payload per replica, each with its own slot array, left claimed
    slots, ids, g, cnt, idx, dy = [], [], [], [], [], []
    for s in range(R):
        slots.append([torch.full((rows,), -1, dtype=torch.int32, device=dev) for rows, _ in MERGE_SPECS])
        ids.append([torch.zeros(B_REP, dtype=torch.int32, device=dev) for _ in MERGE_SPECS])
        g.append([torch.zeros(B_REP * D, dtype=torch.float32, device=dev) for _, D in MERGE_SPECS])
        cnt.append([torch.zeros(1, dtype=torch.int32, device=dev) for _ in MERGE_SPECS])
        idx.append([torch.randint(0, rows, (B_REP, 1), device=dev) for rows, _ in MERGE_SPECS])
        dy.append([torch.randn(B_REP, D, device=dev) for _, D in MERGE_SPECS])
        cid = [torch.empty(B_REP, dtype=torch.int32, device=dev) for _ in MERGE_SPECS]
        K.C().sdp_coalesce(W0, idx[s], dy[s], Ds, [1.0] * n, [0] * n, slots[s], cid, ids[s], g[s], cnt[s])
    torch.cuda.synchronize()
    # the 5000-row table has rows seen by exactly one replica and rows seen by several
    seen = torch.zeros(MERGE_SPECS[0][0], dtype=torch.int64, device=dev)
    for s in range(R):
        seen[torch.unique(idx[s][0])] += 1
    assert int((seen == 1).sum().item()) > 0 and int((seen > 1).sum().item()) > 0

    # float64: segments summed before squaring
    w64 = [w.double().clone() for w in W0]
    h64 = [h.double().view(-1).clone() for h in H0]
    orc = []
    for k, (rows, D) in enumerate(MERGE_SPECS):
        uniq, s = _oracle(torch.cat([idx[r][k] for r in range(R)]), torch.cat([dy[r][k] for r in range(R)]), rows, 0, 1.0)
        assert 0 < uniq.numel() <= rows
        _rowwise64(w64[k], h64[k], uniq, s, lr64)
        orc.append((uniq, s))

    def replica(own):
        """The executor's receive buffer: gathered copies of every payload; own payload and slots."""
        W = [w.clone() for w in W0]
        H = [h.clone() for h in H0]
        slot = [t.clone() for t in slots[own]]
        own_ids = [t.clone() for t in ids[own]]
        own_cnt = [t.clone() for t in cnt[own]]
        gi = [t.clone() for s in range(R) for t in ids[s]]
        gg = [t.clone() for s in range(R) for t in g[s]]
        gc = [t.clone() for s in range(R) for t in cnt[s]]
        mcap = [min(rows, R * B_REP) for rows, _ in MERGE_SPECS]
        mids = [torch.zeros(m, dtype=torch.int32, device=dev) for m in mcap]
        mg = [torch.zeros(m * D, dtype=torch.float32, device=dev) for m, D in zip(mcap, Ds)]
        mcount = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in MERGE_SPECS]
        K.C().sdp_rowwise_merge(gi, gg, gc, own_ids, own_cnt, slot, mids, mg, mcount, Ds, R)
        K.C().emb_rowwise_adagrad_apply(W, H, mids, mg, mcount, slot, lr, EPS)
        torch.cuda.synchronize()
        for k in range(n):
            assert int((slot[k] != -1).sum().item()) == 0, "claim slots not released"
            assert int(own_cnt[k].item()) == 0 and int(mcount[k].item()) == 0, "counts not reset"
        return W, H

    Wa, Ha = replica(0)
    Wb, Hb = replica(2)
    for k in range(n):
        assert torch.equal(Wa[k], Wb[k]) and torch.equal(Ha[k], Hb[k]), f"table {k}: replicas differ"
        uniq, s = orc[k]
        _check(f"merge table {k}", Wa[k], Ha[k], w64[k], h64[k], uniq, s, R * B_REP, W0[k], H0[k])


def test_apply_rejects_mismatched_buffers(gpu):
    from flexmi.ops import _kernels as K
    dev = gpu
    W = torch.zeros(8, 4, device=dev)
    H = torch.zeros(8, 1, device=dev)
    ids = torch.zeros(16, dtype=torch.int32, device=dev)
    g = torch.zeros(16 * 4, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    slot = torch.full((8,), -1, dtype=torch.int32, device=dev)
    lr = torch.tensor([LR], device=dev)
    with pytest.raises(RuntimeError):     # H of the table's shape, not [rows, 1]
        K.C().emb_rowwise_adagrad_apply([W], [torch.zeros(8, 4, device=dev)], [ids], [g], [cnt], [slot], lr, EPS)
    with pytest.raises(RuntimeError):     # H one-dimensional
        K.C().emb_rowwise_adagrad_apply([W], [torch.zeros(8, device=dev)], [ids], [g], [cnt], [slot], lr, EPS)
    with pytest.raises(RuntimeError):     # payload shorter than ids x D
        K.C().emb_rowwise_adagrad_apply([W], [H], [ids], [g[:8]], [cnt], [slot], lr, EPS)
    with pytest.raises(RuntimeError):     # fewer slots than rows
        K.C().emb_rowwise_adagrad_apply([W], [H], [ids], [g], [cnt], [slot[:4]], lr, EPS)


# ------------------------------------------------------------------ model level
B_MODEL = 128


def _dlrm_run(dev, use_graph=False):
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, RowwiseAdagradOptimizer
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
    m.compile(RowwiseAdagradOptimizer(m, lr=0.05, initial_accumulator_value=0.1), LossType.LOSS_BINARY_CROSSENTROPY,
              [MetricsType.METRICS_ACCURACY])
    ex = m.init_layers()
    tables = [ex.wentries[op.weights[0].guid] for op in m.layers if op.op_type == OperatorType.OP_EMBEDDING]
    assert len(tables) == len(dcfg.embedding_size)
    for e in tables:
        assert e.sparse and e.grad is None and set(e.state) == {"h"} and tuple(e.state["h"].shape) == (e.shape[0], 1)
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
def test_dlrm_tiny_rowwise_gpu_matches_cpu(gpu, cpu_dlrm, use_graph):
    ws, loss, hs, sp = _dlrm_run("gpu", use_graph)
    for a, b in zip(cpu_dlrm[0], ws):
        assert np.abs(a - b).max() < 3e-2 * max(1.0, np.abs(a).max()), (a.shape,)
    assert abs(cpu_dlrm[1] - loss) < 2e-2
    for h, idx in zip(hs, sp):
        assert h.shape[1] == 1
        h = h[:, 0]
        untouched = np.ones(h.shape[0], bool)
        untouched[idx.reshape(-1)] = False
        assert h.min() >= np.float32(0.1) and h[~untouched].max() > np.float32(0.1)   # the accumulators moved
        assert np.all(h[untouched] == np.float32(0.1))                                # ... on looked-up rows only
