"""Grouped split-K launch of the split-bf16 fp32 GEMM (csrc/kernels/gemm_x3.hip
fm_gemm_x3v2_grouped_kernel, gemm_f32.hip fm_gemm_f32_grouped): several small-grid problems in one
grid and one reduce.  Each member must be bit-identical to the single GEMM of the same form (256x128
tile) and split depth, and within the fp32 test tolerance of a float64 oracle; the host planner
(csrc/runtime/gemm_group_plan.h) is checked without a GPU; the executor's FM_DW_GROUP plumbing trains
the same weights as the per-layer path, eager and under hipGraph capture."""
import numpy as np
import pytest
import torch

from tests.test_gpu_fp32 import TOL, rel_err

# (M, N, K): a partial last m-tile (480 = 256 + 224); ktiles = 7, so the last split runs fewer k steps;
# ktiles = 3 < 4, so a forced depth of 4 is clamped to 3
SHAPES = [(480, 256, 256), (256, 128, 224), (64, 192, 96)]
FORM4 = 4 << 8


def _operands(gpu, a_k, b_k):
    g = torch.Generator(device="cpu").manual_seed(11)
    out = []
    for M, N, K in SHAPES:
        A = torch.randn(M, K, generator=g).to(gpu)
        B = torch.randn(K, N, generator=g).to(gpu)
        C0 = torch.randn(M, N, generator=g).to(gpu)
        out.append(dict(M=M, N=N, K=K, A=A, B=B, C0=C0, ref=A.double() @ B.double(),
                        Ag=A.contiguous() if a_k else A.t().contiguous(),
                        Bg=B.t().contiguous() if b_k else B.contiguous()))
    return out


@pytest.fixture(scope="module")
def dw_ops(gpu):
    return _operands(gpu, False, False)


def _check_group(Kk, ops, a_k, b_k, ks, beta, rowsum):
    gpu = ops[0]["A"].device
    Cg = [o["C0"].clone() for o in ops]
    Cs = [o["C0"].clone() for o in ops]
    rg = [torch.zeros(o["M"], device=gpu) if rowsum else None for o in ops]
    rs = [torch.zeros(o["M"], device=gpu) if rowsum else None for o in ops]
    mem = [(o["Ag"], o["K"] if a_k else o["M"], o["Bg"], o["K"] if b_k else o["N"], c, o["N"], o["M"], o["N"], o["K"],
            beta, r) for o, c, r in zip(ops, Cg, rg)]
    depths = Kk.gemm_grouped(mem, a_k, b_k, force=ks)
    assert depths == [min(ks, o["K"] // 32) for o in ops], depths
    for o, cg, cs, r1, r2, d in zip(ops, Cg, Cs, rg, rs, depths):
        M, N, K = o["M"], o["N"], o["K"]
        got = Kk.gemm(o["Ag"], K if a_k else M, a_k, o["Bg"], K if b_k else N, b_k, cs, N, M, N, K, beta=beta,
                      rowsum_a=r2, ksplit=d | FORM4)
        assert got == d and Kk.C().gemm_f32_last_form() == 4
        assert torch.equal(cg, cs), (M, N, K, ks, (cg - cs).abs().max().item())
        assert rel_err(cg - (o["C0"] if beta else 0), o["ref"]) < TOL
        if rowsum:
            want = o["A"].double().sum(1)
            assert rel_err(r1, want) < TOL and rel_err(r2, want) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("rowsum", [False, True])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("ks", [1, 2, 4])
def test_grouped_matches_single_and_oracle(gpu, dw_ops, ks, beta, rowsum):
    from flexmi.ops import _kernels as Kk
    n0 = Kk.C().gemm_f32_grouped_count()
    _check_group(Kk, dw_ops, False, False, ks, beta, rowsum)
    assert Kk.C().gemm_f32_grouped_count() == n0 + 1


@pytest.mark.gpu
def test_grouped_forward_orientation(gpu):
    """K-contiguous A and B (the forward orientation): the grouping does not depend on the orientation."""
    from flexmi.ops import _kernels as Kk
    _check_group(Kk, _operands(gpu, True, True), True, True, 2, True, False)


@pytest.mark.gpu
def test_grouped_deep_reduce_order(gpu):
    """Depth 16: the single GEMM reduces quads in fm_gemm_reduce_deep's interleaved order (and an N that is
    no multiple of 4 one output at a time, in slab order); the grouped reduce must add in the same orders."""
    from flexmi.ops import _kernels as Kk
    g = torch.Generator(device="cpu").manual_seed(13)
    mem, single, refs = [], [], []
    for M, N, K in [(256, 128, 1024), (128, 256, 512), (64, 130, 512)]:
        A, B = torch.randn(K, M, generator=g).to(gpu), torch.randn(K, N, generator=g).to(gpu)
        C0 = torch.randn(M, N, generator=g).to(gpu)
        mem.append((A, M, B, N, C0.clone(), N, M, N, K, True, None))
        single.append(C0.clone())
        refs.append(A.double().t() @ B.double() + C0.double())
    assert Kk.gemm_grouped(mem, False, False, force=16) == [16, 16, 16]
    for m, cs, ref in zip(mem, single, refs):
        A, _, B, _, cg, _, M, N, K = m[:9]
        assert Kk.gemm(A, M, False, B, N, False, cs, N, M, N, K, beta=True, ksplit=16 | FORM4) == 16
        assert torch.equal(cg, cs), (M, N, K, (cg - cs).abs().max().item())
        assert rel_err(cg, ref) < TOL


@pytest.mark.gpu
def test_grouped_shared_output_is_not_raced(gpu):
    """Two members accumulating into ONE output (two layers sharing a weight): the kernel takes only the
    first of them, so no two concurrently reduced problems write the same C; the wrapper's caller runs the other."""
    from flexmi.ops import _kernels as Kk
    g = torch.Generator(device="cpu").manual_seed(17)
    M, N, K = 256, 128, 256
    A = [torch.randn(K, M, generator=g).to(gpu) for _ in range(3)]
    B = [torch.randn(K, N, generator=g).to(gpu) for _ in range(3)]
    shared, own = torch.zeros(M, N, device=gpu), torch.zeros(M, N, device=gpu)
    mem = [(A[0], M, B[0], N, shared, N, M, N, K, True, None), (A[1], M, B[1], N, shared, N, M, N, K, True, None),
           (A[2], M, B[2], N, own, N, M, N, K, True, None)]
    assert Kk.gemm_grouped(mem, False, False, force=2) == [2, 0, 2]
    assert Kk.gemm_grouped(mem[1:], False, False, force=2) == [2, 2] and Kk.gemm_grouped(mem[:2], False, False, force=2) == [0, 0]


def _dw_calls(gpu, n, width, batch, tied=()):
    """linear_backward "dw" argument tuples of n width x width layers at one batch; layer j of every pair
    (i, j) in ``tied`` accumulates into layer i's dW and db (a shared weight)."""
    g = torch.Generator(device="cpu").manual_seed(19)
    calls, want = [], {}
    dws = [torch.zeros(width, width, device=gpu) for _ in range(n)]
    dbs = [torch.zeros(width, device=gpu) for _ in range(n)]
    for i, j in tied:
        dws[j], dbs[j] = dws[i], dbs[i]
    for k in range(n):
        x, dpre = torch.randn(batch, width, generator=g).to(gpu), torch.randn(batch, width, generator=g).to(gpu)
        w = torch.empty(width, width, device=gpu)
        # (x2, w, y2, dy2, act, dx2, dx_acc, dw, db, ws, grad_is_dpre, fuse_below, phase, upd)
        calls.append((x, w, dpre, dpre, 10, None, False, dws[k], dbs[k], {}, True, None, "dw", None))
        key = dws[k].data_ptr()
        gw, gb = dpre.double().t() @ x.double(), dpre.double().sum(0)
        want[key] = (dws[k], dbs[k], want[key][2] + gw, want[key][3] + gb) if key in want else (dws[k], dbs[k], gw, gb)
    return calls, list(want.values())


@pytest.mark.gpu
@pytest.mark.parametrize("n,tied,grouped,launches", [(4, [(0, 1)], 3, 1), (6, [(0, 1), (2, 3)], 6, 2)])
def test_dw_group_tied_layers(gpu, n, tied, grouped, launches):
    """512-wide layers at batch 512, some sharing a weight (one gradient buffer, contributions summed): a
    launch holds one member per buffer; the other joins the next launch, or runs alone when none is left to
    pair it with.  Four layers: 0, 2, 3 grouped, 1 alone.  Six: 0, 2, 4, 5, then 1 and 3."""
    from flexmi.ops import _kernels as Kk
    calls, want = _dw_calls(gpu, n, 512, 512, tied=tied)
    n0 = Kk.C().gemm_f32_grouped_count()
    assert Kk.linear_dw_group(calls) == grouped
    assert Kk.C().gemm_f32_grouped_count() == n0 + launches
    assert len(want) == n - len(tied)
    for dw, db, gw, gb in want:
        assert rel_err(dw, gw) < TOL and rel_err(db, gb) < TOL


@pytest.mark.gpu
def test_dw_group_more_layers_than_a_launch_takes(gpu):
    """18 groupable layers in one flush: launches of four (and a last one of two), every gradient right."""
    from flexmi.ops import _kernels as Kk
    calls, want = _dw_calls(gpu, 18, 512, 512)
    n0 = Kk.C().gemm_f32_grouped_count()
    assert Kk.linear_dw_group(calls) == 18
    assert Kk.C().gemm_f32_grouped_count() == n0 + 5
    for dw, db, gw, gb in want:
        assert rel_err(dw, gw) < TOL and rel_err(db, gb) < TOL


@pytest.mark.gpu
def test_grouped_declines(gpu):
    """One eligible member, or members outside the big-GEMM policy without a forced depth: nothing is
    launched and every depth is 0 (the caller runs the members itself)."""
    from flexmi.ops import _kernels as Kk
    ops = _operands(gpu, False, False)
    mem = [(o["Ag"], o["M"], o["Bg"], o["N"], o["C0"].clone(), o["N"], o["M"], o["N"], o["K"], False, None) for o in ops]
    n0 = Kk.C().gemm_f32_grouped_count()
    assert Kk.gemm_grouped(mem, False, False) == [0, 0, 0]
    assert Kk.gemm_grouped(mem[:1], False, False, force=2) == [0]
    assert Kk.C().gemm_f32_grouped_count() == n0
    for m, o in zip(mem, ops):
        assert torch.equal(m[4], o["C0"])


# ---------------------------------------------------------------- planner (no GPU)
MLPERF = ([512, 1024, 1024], [1024, 1024, 480], [8192, 8192, 8192])     # dW of 1024->512, 1024->1024, 480->1024


def _tiles(M, N):
    return ((M + 255) // 256) * ((N + 127) // 128)


def test_planner_mlperf_triple(native):
    M, N, K = MLPERF
    ks, first, off, total, where = native.gemm_group_plan(M, N, K, 256, 64 << 20)
    assert ks == [4, 4, 4] and first == [0, 64, 192, 256] and len(where) == 256
    assert total == sum(4 * m * n * 4 for m, n in zip(M, N))           # 31.5 MiB of slabs, written once


@pytest.mark.parametrize("shapes,cus,force", [(MLPERF, 256, 0), (MLPERF, 304, 0), (MLPERF, 256, 2),
                                              (([480, 256, 64], [256, 128, 192], [256, 224, 96]), 256, 4),
                                              (([512, 512, 300, 2048], [480, 512, 130, 256], [512, 512, 8192, 1024]), 256, 0)])
def test_planner_covers_every_tile_split_once(native, shapes, cus, force):
    M, N, K = shapes
    ks, first, off, total, where = native.gemm_group_plan(M, N, K, cus, 64 << 20, force)
    want = sorted((g, t, s) for g in range(len(M)) for t in range(_tiles(M[g], N[g])) for s in range(ks[g]))
    assert sorted(where) == want                      # every (problem, tile, split) exactly once
    assert first[-1] == len(where) and (force or len(where) <= cus)
    for b, (g, t, s) in enumerate(where):             # tile fastest inside its problem's block range
        assert first[g] <= b < first[g + 1] and b - first[g] == s * _tiles(M[g], N[g]) + t
    for g in range(len(M)):
        kt = K[g] // 32
        assert 1 <= ks[g] <= (min(force, kt) if force else min(16, kt // 4))
    end = 0
    for g in range(len(M)):                           # slab ranges: disjoint, 16-B aligned, inside the total
        size = ks[g] * M[g] * N[g] * 4 if ks[g] > 1 else 0
        assert off[g] % 16 == 0 and off[g] >= end
        end = off[g] + size
    assert end <= total


def test_planner_not_grouped(native):
    M, N, K = MLPERF
    assert native.gemm_group_plan(M[:1], N[:1], K[:1], 256, 64 << 20) is None          # one problem
    assert native.gemm_group_plan(M, N, K, 64, 64 << 20) is None                       # the tiles fill the device
    need = sum(4 * m * n * 4 for m, n in zip(M, N))
    assert native.gemm_group_plan(M, N, K, 256, need - 16) is None                     # workspace too small
    assert native.gemm_group_plan(M, N, K, 100, 64 << 20) is None                      # no common depth above 1 fits
    assert native.gemm_group_plan(M, N, K, 256, need) is not None


# ---------------------------------------------------------------- executor
def _train_mlp(monkeypatch, group, graph, tied=False):
    from flexmi.core import FFConfig, FFModel, SGDOptimizer, LossType, MetricsType
    from flexmi.core.types import ActiMode
    from flexmi.ops import _kernels as Kk
    monkeypatch.setenv("FM_DW_GROUP", "1" if group else "0")
    cfg = FFConfig()
    cfg.batchSize = B = 512
    cfg.seed = 5
    cfg.compute_dtype = "fp32"
    m = FFModel(cfg)
    x = m.create_tensor([B, 480], name="x")
    h = m.dense(x, 512, ActiMode.AC_MODE_RELU, name="fc1")
    h = m.dense(h, 512, ActiMode.AC_MODE_RELU, name="fc2")
    if tied:            # fc2's weight used twice: both dW GEMMs accumulate into one gradient buffer
        h = m.dense(h, 512, ActiMode.AC_MODE_RELU, shared_op=h.owner_op, name="fc2_tied")
    m.dense(h, 8, name="fc3")
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [MetricsType.METRICS_MEAN_SQUARED_ERROR])
    ex = m.init_layers()
    rng = np.random.RandomState(7)
    ex.scatter_from_host(x, rng.rand(B, 480).astype(np.float32))
    lab = m.get_label_tensor()
    ex.scatter_from_host(lab, rng.rand(*lab.dims).astype(np.float32))
    n0 = Kk.C().gemm_f32_grouped_count()
    ex.train_step()
    per_step = Kk.C().gemm_f32_grouped_count() - n0
    if graph:
        run = ex.capture_step()
        for _ in range(2):
            run()
    else:
        for _ in range(2):
            ex.train_step()
    torch.cuda.synchronize()
    return [w.get_weights(m) for w in m.parameters], per_step


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_executor_dw_group_matches_ungrouped(gpu, monkeypatch, graph):
    """480 -> 512 -> 512 -> 8 at batch 512: two dW GEMMs the split kernel takes (512 x 480 and 512 x 512,
    K = 512) and one it does not; 3 SGD steps."""
    ref, n_off = _train_mlp(monkeypatch, False, graph)
    got, n_on = _train_mlp(monkeypatch, True, graph)
    assert n_off == 0 and n_on == 1, (n_off, n_on)          # one grouped launch a step
    for a, b in zip(ref, got):
        assert rel_err(torch.from_numpy(np.asarray(a)), torch.from_numpy(np.asarray(b))) < TOL, a.shape


@pytest.mark.gpu
def test_executor_dw_group_tied_weight(gpu, monkeypatch):
    """480 -> 512 -> 512 -> (the same 512 x 512 weight again) -> 8: the two layers sharing a weight never sit
    in one grouped launch, and the summed gradient trains the same weights as the per-layer path."""
    ref, n_off = _train_mlp(monkeypatch, False, False, tied=True)
    got, n_on = _train_mlp(monkeypatch, True, False, tied=True)
    assert n_off == 0 and n_on == 1, (n_off, n_on)
    assert len(ref) == len(got) == 6                         # fc1, fc2 (shared), fc3: weight + bias each
    for a, b in zip(ref, got):
        assert rel_err(torch.from_numpy(np.asarray(a)), torch.from_numpy(np.asarray(b))) < TOL, a.shape
