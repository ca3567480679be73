"""csrc/kernels/act_gemm.hip: the fused dense + GELU / tanh-GELU / SiLU forward, fm_act_bwd and the unary codes 5-7 against
fp64 evaluated from the stored rounded pre-activation, and ActLinear on the GPU against the CPU backend in both forms."""
import pytest
import torch
import torch.nn.functional as F

from flexmi.core.types import ActiMode

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}     # max-normalised, as tests/test_gpu_gated.py
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
ACTS = {"gelu": (ActiMode.AC_MODE_GELU, 5), "gelu_tanh": (ActiMode.AC_MODE_GELU_TANH, 6), "silu": (ActiMode.AC_MODE_SILU, 7)}


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def act64(z, act, grad=False):
    """fp64 act(z), or act'(z) by autograd"""
    z = z.double().cpu().clone().requires_grad_(grad)
    a = F.silu(z) if act == "silu" else F.gelu(z, approximate="tanh" if act == "gelu_tanh" else "none")
    return torch.autograd.grad(a.sum(), z)[0] if grad else a


def _op(act, M, H, FF, bias=True):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = "cpu", "fp32", M
    m = FFModel(cfg)
    return m.dense(m.create_tensor([M, H]), FF, ACTS[act][0], bias).owner_op


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("M,FF,H,sliced", [(1, 4, 8, False), (128, 128, 64, False), (256, 256, 192, False),
                                          (130, 132, 136, False), (130, 132, 136, True)])
def test_fused_forward_against_fp64(gpu, monkeypatch, M, FF, H, sliced, act, bias):
    from flexmi.ops import act_linear
    from flexmi.ops.base import OpCtx
    monkeypatch.setattr(act_linear, "FORM", "fused")
    g = torch.Generator().manual_seed(M + FF + H)
    x = (torch.randn(M, H, generator=g) * (2 / H ** 0.5)).bfloat16()          # z ~ N(0, 2^2): both tails of the activations
    w, b = torch.randn(FF, H, generator=g).bfloat16(), torch.randn(FF, generator=g)
    xbuf = torch.zeros(M, H + (24 if sliced else 0), dtype=torch.bfloat16, device="cuda")
    ybuf = torch.full((M, FF + (16 if sliced else 0)), float("nan"), dtype=torch.bfloat16, device="cuda")
    xs, ys = (xbuf[:, 8:8 + H], ybuf[:, 8:8 + FF]) if sliced else (xbuf, ybuf)
    xs.copy_(x)
    ctx = OpCtx(_op(act, M, H, FF, bias), 0, "hip", torch.bfloat16)
    ctx.inputs, ctx.weights, ctx.wcompute, ctx.outputs = [xs], [w.float().cuda(), b.cuda()][:1 + bias], [w.cuda()], [ys]
    ctx.saved["pre"] = torch.full((M, FF), float("nan"), dtype=torch.bfloat16, device="cuda")
    ctx.op.forward(ctx)
    pre = ctx.saved["pre"]
    assert rel_err(pre, x.double() @ w.double().t() + (b.double() if bias else 0)) < 1e-2, "pre"
    assert rel_err(ys, act64(pre, act)) < 1e-2, "y"
    assert not sliced or torch.isnan(torch.cat([ybuf[:, :8], ybuf[:, 8 + FF:]], 1)).all(), "the padding of y was written"


@pytest.mark.parametrize("act", list(ACTS))
@DTYPES
@pytest.mark.parametrize("M,FF", [(3, 4), (33, 20), (70, 264), (None, 24)], ids=["3x4", "33x20", "70x264", "blocks"])
def test_act_bwd_against_fp64(gpu, M, FF, dt, act):
    from flexmi.ops import _kernels as K
    M = M or 2 * K.act_bwd_rows() + 3                                          # three blocks give partial rows of db
    g = torch.Generator().manual_seed(M + FF)
    pre = torch.randn(M, FF, generator=g) * 2
    pre[0, :4] = torch.tensor([-1.2785, -1.2780, -0.7520, -0.7515])           # either side of the roots of silu' and gelu'
    pre, dy, db0 = pre.to(dt).cuda(), torch.randn(M, FF, generator=g).to(dt).cuda(), torch.randn(FF, generator=g).cuda()
    out = []
    for _ in range(2):
        dpre, db = torch.full((M, FF), float("nan"), dtype=dt, device="cuda"), db0.clone()
        K.act_bwd(dy, pre, dpre, db, ACTS[act][1])
        out.append((dpre, db))
    dz64 = dy.double().cpu() * act64(pre, act, grad=True)
    assert rel_err(out[0][0], dz64) < TOL[dt], "dz"
    assert rel_err(out[0][1], db0.double().cpu() + dz64.sum(0)) < TOL[dt], "db"
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0]), "db differs between two calls"


def _run(backend, dt, act, acc, tensors):
    """one forward and backward of an ActLinear on its OpCtx: y, pre, dx, dw, db"""
    from flexmi.ops.base import OpCtx
    dev = "cuda" if backend == "hip" else "cpu"
    x, w, b, dy, dx0 = [t.to(dev) for t in tensors]
    M, H, FF = x.shape[0], x.shape[1], w.shape[0]
    c = OpCtx(_op(act, M, H, FF), 0, backend, dt)
    c.inputs, c.weights, c.wcompute, c.outputs = [x.to(dt)], [w, b], [w.to(dt)], [torch.zeros(M, FF, dtype=dt, device=dev)]
    c.op.forward(c)
    c.out_grads, c.in_grads, c.in_grad_accumulate = [dy.to(dt)], [dx0.to(dt).clone()], [acc]
    c.weight_grads = [torch.zeros(FF, H, device=dev), torch.zeros(FF, device=dev)]
    c.op.backward(c)
    return c.outputs[0], c.saved["pre"], c.in_grads[0], c.weight_grads[0], c.weight_grads[1]


@pytest.mark.parametrize("dt,form,act,acc,M,FF,H", [
    (torch.bfloat16, "fused", "gelu", True, 129, 136, 72), (torch.bfloat16, "composed", "gelu_tanh", False, 129, 136, 72),
    (torch.float32, "composed", "silu", True, 129, 136, 72), (torch.bfloat16, "auto", "gelu", False, 33, 10, 20)],
    ids=["bf16-fused", "bf16-composed", "fp32-composed", "bf16-auto-refused"])
def test_op_gpu_matches_cpu(gpu, monkeypatch, dt, form, act, acc, M, FF, H):
    from flexmi.ops import act_linear
    monkeypatch.setattr(act_linear, "FORM", form)
    g = torch.Generator().manual_seed(2)
    tensors = [torch.randn(s, generator=g) * k for s, k in zip(((M, H), (FF, H), (FF,), (M, FF), (M, H)), (1, H ** -0.5, 1, 1, 1))]
    cpu, hip = _run("cpu", dt, act, acc, tensors), _run("hip", dt, act, acc, tensors)
    for name, c, h in zip(("y", "pre", "dx", "dw", "db"), cpu, hip):
        assert rel_err(h, c) < TOL[dt], name


@pytest.mark.parametrize("act", list(ACTS))
@DTYPES
@pytest.mark.parametrize("n", [1, 7, 8, 2053])
def test_unary_codes_against_fp64(gpu, n, dt, act):
    from flexmi.ops import _kernels as K
    g = torch.Generator().manual_seed(n)
    x, dy, dx0 = ((torch.randn(n, generator=g) * 2).to(dt).cuda() for _ in range(3))
    y, dx = torch.full_like(x, float("nan")), dx0.clone()
    K.unary_forward(ACTS[act][1], x, y)
    K.unary_backward(ACTS[act][1], x, y, dy, dx, True)
    assert rel_err(y, act64(x, act)) < TOL[dt]
    assert rel_err(dx, dx0.double().cpu() + dy.double().cpu() * act64(x, act, grad=True)) < TOL[dt]
