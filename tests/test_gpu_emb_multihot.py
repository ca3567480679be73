"""The work-balanced multi-table embedding forward (``fm_emb_fwd_balanced``, csrc/kernels/embedding.hip)
for launch sets whose tables have unequal bag sizes: against a float64 oracle and bit for bit against
the per-table-grid kernels (``embedding_set_fwd_mode``), across the 32-table descriptor boundary, the
scalar fallback, under hipGraph capture, and ``tiny_dcn_multihot`` on the GPU against the CPU executor.
Every case asserts through ``embedding_fwd_last_form()`` that it ran the kernel it means to test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a = a.double()
    b = b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _tol(dt):      # the float64-oracle tolerance of test_gpu_kernels.py::test_embedding_fwd_long_bag_split
    return 1e-5 if dt == torch.float32 else 1e-2


def _oracle(W, idx, lo, scale):
    r = idx.long() - lo
    ok = (r >= 0) & (r < W.shape[0])
    return (W.double()[r.clamp(0, W.shape[0] - 1)] * ok[..., None]).sum(1) * scale


def _indices(gpu, B, rows, bag, lo, dtype, gen):
    """Uniform lookups over the whole table (so a row shard sees lookups it does not hold), plus an index
    of -1, one past the table and a bag that holds one row twice."""
    idx = torch.randint(0, rows + lo, (B, bag), generator=gen, device=gpu).to(dtype)
    if B >= 3:
        idx[0, 0] = -1
        idx[1, bag - 1] = rows + lo + 3
        if bag > 1:
            idx[2, 1] = idx[2, 0]
    return idx


class _Set:
    """Tables (rows, D, bag, lo, idx dtype, scale, ld, col): output i is the column slice [col, col + D)
    of a [B, ld] buffer filled with a sentinel."""

    SENT = 7.0

    def __init__(self, gpu, B, specs, seed, weights=None):
        gen = torch.Generator(device=gpu).manual_seed(seed)
        self.gpu, self.B, self.specs = gpu, B, specs
        self.W = [(weights or (lambda r, D: torch.randn(r, D, generator=gen, device=gpu)))(r, D)
                  for r, D, *_ in specs]
        self.idx = [_indices(gpu, B, r, bag, lo, dt, gen) for r, D, bag, lo, dt, *_ in specs]

    def run(self, out_dt):
        from flexmi.ops import _kernels as Kk
        bufs = [torch.full((self.B, ld), self.SENT, device=self.gpu, dtype=out_dt) for *_, ld, col in self.specs]
        outs = [b.view(-1)[col:] for b, (*_, col) in zip(bufs, self.specs)]
        Kk.C().embedding_fwd_multi(self.W, self.idx, outs, [s[6] for s in self.specs], [s[5] for s in self.specs],
                                   [s[3] for s in self.specs])
        torch.cuda.synchronize()
        return bufs

    def check(self, bufs, out_dt):
        for W, idx, b, (r, D, bag, lo, dt, scale, ld, col) in zip(self.W, self.idx, bufs, self.specs):
            assert rel_err(b[:, col:col + D], _oracle(W, idx, lo, scale)) < _tol(out_dt), (r, D, bag, lo)
            rest = torch.cat([b[:, :col], b[:, col + D:]], 1)
            assert bool((rest == self.SENT).all()), (r, D, bag, "columns outside the slice")


def _spec(rows, D, bag, lo=0, dt=torch.int64, scale=1.0, ld=None, col=0):
    return (rows, D, bag, lo, dt, scale, D if ld is None else ld, col)


@pytest.fixture
def fwd_mode():
    from flexmi.ops import _kernels as Kk
    try:
        yield Kk.embedding_set_fwd_mode
    finally:
        Kk.embedding_set_fwd_mode(0)


MIXED = [_spec(5000, 128, 1), _spec(50, 128, 3, ld=200, col=40), _spec(4000, 128, 100), _spec(300, 16, 7, scale=1.0 / 7),
         _spec(5000, 128, 27, lo=1000), _spec(9, 256, 5), _spec(20, 24, 2),
         _spec(1000, 128, 1, dt=torch.int32), _spec(700, 64, 4, dt=torch.int32)]


@pytest.mark.parametrize("out_dt", [torch.float32, torch.bfloat16])
def test_unequal_bags_run_balanced_and_equal_the_table_grid_kernel(gpu, fwd_mode, out_dt):
    """B = 333 is no multiple of any rows-per-iteration (2, 4, 8, 42, 64); launch sets form per index
    width, so each width has unequal bags."""
    from flexmi.ops import _kernels as Kk
    s = _Set(gpu, 333, MIXED, seed=5)
    fwd_mode(0)
    got = s.run(out_dt)
    assert Kk.embedding_fwd_last_form() == "balanced"
    s.check(got, out_dt)
    fwd_mode(1)
    old = s.run(out_dt)
    assert Kk.embedding_fwd_last_form() == "multi"
    s.check(old, out_dt)
    for a, b, sp in zip(got, old, MIXED):
        assert torch.equal(a, b), sp


def test_int32_indices_through_the_chunked_bag_loop(gpu, fwd_mode):
    """The set above has int32 bags of 1 and 4 only (the all-in-flight paths): bags of 9 and 33 take the
    chunked loop with int32 indices, an odd and an even number of chunks."""
    from flexmi.ops import _kernels as Kk
    i32 = torch.int32
    s = _Set(gpu, 70, [_spec(900, 32, 9, dt=i32), _spec(50, 128, 2, dt=i32), _spec(3000, 64, 33, lo=500, dt=i32)], seed=12)
    fwd_mode(0)
    got = s.run(torch.bfloat16)
    assert Kk.embedding_fwd_last_form() == "balanced"
    s.check(got, torch.bfloat16)
    fwd_mode(1)
    old = s.run(torch.bfloat16)
    assert Kk.embedding_fwd_last_form() == "multi"
    for a, b in zip(got, old):
        assert torch.equal(a, b)


@pytest.mark.parametrize("out_dt", [torch.float32, torch.bfloat16])
def test_mode2_on_uniform_sets_equals_su_and_split(gpu, fwd_mode, out_dt):
    """Uniform sets keep their kernels in mode 0; mode 2 forces the balanced one, bit for bit equal.
    The balanced kernel adds in ascending bag order like fm_emb_fwd_multi; fm_emb_fwd_split adds four
    interleaved partial sums, so against it the tables hold multiples of 1/4 in [-2, 2]: every sum of
    20 of them is exact in fp32 in any order, and bit equality then checks the lookups, the
    predication, the scale and the one rounding of the store.  With random weights a bag-20 set is
    checked against the oracle and bit for bit against mode 1's fm_emb_fwd_multi (same order of additions)."""
    from flexmi.ops import _kernels as Kk
    torch.manual_seed(3)
    quarters = lambda r, D: torch.randint(-8, 9, (r, D), device=gpu).float() / 4
    cases = [(_Set(gpu, 333, [_spec(5000, 128, 1), _spec(40, 128, 1), _spec(700, 64, 1, lo=100)], seed=6), "multi_su"),
             (_Set(gpu, 37, [_spec(5000, 128, 20), _spec(5000, 128, 20, scale=1.0 / 20), _spec(5000, 128, 20, lo=1000)],
                   seed=7, weights=quarters), "split")]
    for s, form in cases:
        fwd_mode(0)
        ref = s.run(out_dt)
        assert Kk.embedding_fwd_last_form() == form
        s.check(ref, out_dt)
        fwd_mode(2)
        got = s.run(out_dt)
        assert Kk.embedding_fwd_last_form() == "balanced"
        for a, b in zip(got, ref):
            assert torch.equal(a, b), form
    # random weights; one table of another D keeps mode 1 off the split kernel (it wants one D)
    s = _Set(gpu, 37, [_spec(5000, 128, 20), _spec(5000, 128, 20, scale=1.0 / 20), _spec(5000, 64, 20, lo=1000)], seed=8)
    fwd_mode(2)
    got = s.run(out_dt)
    assert Kk.embedding_fwd_last_form() == "balanced"
    s.check(got, out_dt)
    fwd_mode(1)
    old = s.run(out_dt)
    assert Kk.embedding_fwd_last_form() == "multi"
    for a, b in zip(got, old):
        assert torch.equal(a, b)


@pytest.mark.parametrize("out_dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("idx_dt", [torch.int64, torch.int32])
@pytest.mark.parametrize("bag,form", [(1, "multi_su"), (11, "multi"), (20, "split")])
def test_uniform_forms_on_batches_that_end_inside_a_block_iteration(gpu, fwd_mode, bag, form, idx_dt, out_dt):
    """The per-table-grid forms share their lookup loops (emb_bal_short, emb_gather_sum): B = 37 and
    B = 2085 are no multiple of the samples a block iteration covers at D = 128 or D = 64 (8 / 16 lane
    groups, times four samples in the single-lookup loop, over 1 to 4 groups per sample in the split
    kernel), so the clamped loads and the b >= B exits run.  A bag of 11 is one eight-wide gather
    and a tail of three; every set holds an index of -1 and one past the table, and a row shard."""
    from flexmi.ops import _kernels as Kk
    fwd_mode(0)
    for B in (37, 2085):
        for D in (128, 64):
            s = _Set(gpu, B, [_spec(5000, D, bag, dt=idx_dt), _spec(3000, D, bag, lo=1000, dt=idx_dt, scale=0.5)],
                     seed=B + D + bag)
            got = s.run(out_dt)
            assert Kk.embedding_fwd_last_form() == form, (B, D)
            s.check(got, out_dt)


@pytest.mark.parametrize("B", [5, 1])
def test_descriptor_batches_of_32(gpu, fwd_mode, B):
    """34 tables: a launch set of 32 and one of 2, both with unequal bags."""
    from flexmi.ops import _kernels as Kk
    s = _Set(gpu, B, [_spec(64, 32, (1, 2, 3, 5)[k % 4]) for k in range(34)], seed=9)
    fwd_mode(0)
    got = s.run(torch.float32)
    assert Kk.embedding_fwd_last_form() == "balanced"
    s.check(got, torch.float32)


def test_non_vectorisable_table_falls_back_to_scalar(gpu, fwd_mode):
    from flexmi.ops import _kernels as Kk
    s = _Set(gpu, 333, [_spec(500, 128, 3), _spec(60, 6, 2), _spec(900, 64, 9)], seed=10)
    for mode in (0, 2):
        fwd_mode(mode)
        got = s.run(torch.float32)
        assert Kk.embedding_fwd_last_form() == "scalar"
        s.check(got, torch.float32)


def test_balanced_launch_is_capturable(gpu, fwd_mode):
    """One linear stream: the launch captured once, replayed with new indices in the same buffers."""
    from flexmi.ops import _kernels as Kk
    specs = [_spec(5000, 128, 1), _spec(50, 128, 3), _spec(4000, 128, 100), _spec(300, 16, 7)]
    s = _Set(gpu, 333, specs, seed=11)
    fwd_mode(0)
    outs = [torch.zeros(333, sp[1], device=gpu) for sp in specs]
    args = (s.W, s.idx, outs, [sp[6] for sp in specs], [sp[5] for sp in specs], [sp[3] for sp in specs])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Kk.C().embedding_fwd_multi(*args)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Kk.C().embedding_fwd_multi(*args)
    assert Kk.embedding_fwd_last_form() == "balanced"
    for k in range(2):
        fresh = _Set(gpu, 333, specs, seed=20 + k)
        for dst, src in zip(s.idx, fresh.idx):
            dst.copy_(src)
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for W, idx, o, sp in zip(s.W, fresh.idx, outs, specs):
            assert rel_err(o, _oracle(W, idx, sp[3], sp[5])) < _tol(torch.float32), (k, sp)


# ------------------------------------------------------------------ tiny_dcn_multihot end to end
@pytest.mark.parametrize("optname", ["sgd", "rowwise_adagrad"])
def test_tiny_dcn_multihot_gpu_matches_cpu(gpu, fwd_mode, optname):
    """Bounds of tests/test_gpu_cross.py::test_tiny_dcn_gpu_matches_cpu."""
    from flexmi.core import FFConfig, FFModel, LossType, MetricsType, RowwiseAdagradOptimizer, SGDOptimizer
    from flexmi.core.types import OperatorType
    from flexmi.models.dlrm import DLRMConfig, build_dlrm
    from flexmi.ops import _kernels as Kk
    B = 64
    fwd_mode(0)
    rng = np.random.RandomState(1)
    dcfg = DLRMConfig.preset("tiny_dcn_multihot")
    dense = rng.rand(B, 13).astype(np.float32)
    sp = [rng.randint(0, r, (B, b)).astype(np.int64) for r, b in zip(dcfg.embedding_size, dcfg.bag_sizes())]
    sp[2][5, 3] = sp[2][5, 0]                                   # one bag holds the same row twice
    lab = rng.randint(0, 2, (B, 1)).astype(np.float32)
    out = {}
    for dev in ("cpu", "gpu"):
        cfg = FFConfig()
        cfg.batchSize, cfg.device, cfg.compute_dtype = B, dev, "fp32"
        m = FFModel(cfg)
        d, s, p = build_dlrm(m, dcfg)
        assert [tuple(t.dims) for t in s] == [(B, 3), (B, 1), (B, 8), (B, 2)]
        opt = SGDOptimizer(m, 0.1) if optname == "sgd" else RowwiseAdagradOptimizer(m, 0.1)
        m.compile(opt, LossType.LOSS_BINARY_CROSSENTROPY, [MetricsType.METRICS_ACCURACY])
        ex = m.init_layers()
        for _ in range(3):
            dd = np.zeros((B, d.dims[1]), np.float32)
            dd[:, :13] = dense
            ex.scatter_from_host(d, dd)
            for t, a in zip(s, sp):
                ex.scatter_from_host(t, a)
            ex.scatter_from_host(m.get_label_tensor(), lab)
            ex.train_step()
        if dev == "gpu":
            torch.cuda.synchronize()
            assert Kk.embedding_fwd_last_form() == "balanced"
            names = [it.name for it in ex.prog_fwd + ex.prog_bwd]
            assert "embedding0.group_fwd" in names
            if optname == "sgd":                                # the existing multi-table backward launch
                assert "embedding0.group_bwd" in names, names
        ws = [w.get_weights(m) for w in m.parameters]
        ws[0] = ws[0][:, :13]   # drop the (unused, zero-input) padding columns of the first layer
        tabs = [i for i, w in enumerate(m.parameters) if w.owner_op.op_type == OperatorType.OP_EMBEDDING]
        out[dev] = (ws, m.get_perf_metrics().get_loss(), tabs)
    assert len(out["cpu"][0]) == len(out["gpu"][0]) == 18 and len(out["gpu"][2]) == 4
    for i, (a, b) in enumerate(zip(out["cpu"][0], out["gpu"][0])):
        assert np.abs(a - b).max() < 3e-2 * max(1.0, np.abs(a).max()), (i, a.shape, i in out["gpu"][2])
    assert abs(out["cpu"][1] - out["gpu"][1]) < 2e-2
