"""The Attention op and ``FFModel.multihead_attention`` on the fp32 CPU executor: the op's forward
and hand-written backward against autograd of the explicit float64 formula, the builder against
``torch.nn.MultiheadAttention`` through three SGD steps, and what build and compile() refuse."""
import numpy as np
import pytest
import torch


def _cpu_model(B, device="cpu"):
    from flexmi.core import FFConfig, FFModel
    cfg = FFConfig()
    cfg.device, cfg.compute_dtype, cfg.batchSize = device, "fp32", B
    return FFModel(cfg)


def attention_f64(q, k, v, heads, causal, scale):
    """softmax(scale q k^T + mask) v per head on [B, T, heads * dh] operands, in float64."""
    B, Tq, E = q.shape
    sp = lambda t: t.double().reshape(B, t.shape[1], heads, E // heads).transpose(1, 2)   # noqa: E731
    s = sp(q) @ sp(k).transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(torch.ones(Tq, k.shape[1], dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(B, Tq, E)


@pytest.mark.parametrize("Tq,Tk,causal,accs,drop", [
    (7, 7, True, (False, False, False), None), (7, 7, False, (True, True, True), None),
    (5, 9, False, (True, False, True), None), (9, 5, False, (False, True, False), 1), (6, 6, True, (True, True, False), 0)])
def test_op_matches_autograd(Tq, Tk, causal, accs, drop):
    from flexmi.ops.base import OpCtx
    B, heads, dh = 2, 3, 4
    E = heads * dh
    m = _cpu_model(B)
    out = m.attention(m.create_tensor([B, Tq, E]), m.create_tensor([B, Tk, E]), m.create_tensor([B, Tk, E]), heads, causal)
    op = out.owner_op
    assert tuple(out.dims) == (B, Tq, E) and op.splittable_dims() == {0} and not op.weights
    g = torch.Generator().manual_seed(3)
    vals = [torch.randn(B, T, E, generator=g, requires_grad=True) for T in (Tq, Tk, Tk)]
    dy = torch.randn(B, Tq, E, generator=g)
    ref = attention_f64(*vals, heads, causal, dh ** -0.5)
    ref.backward(dy.double())

    ctx = OpCtx(op, 0, "cpu", torch.float32)
    ctx.inputs = [x.detach().clone() for x in vals]
    ctx.outputs = [torch.full((B, Tq, E), float("nan"))]
    op.forward(ctx)
    torch.testing.assert_close(ctx.outputs[0], ref.detach().float(), rtol=0, atol=1e-5)
    prev = [torch.randn_like(x) for x in vals]
    ctx.out_grads = [dy.clone()]
    ctx.in_grads = [None if i == drop else p.clone() for i, p in enumerate(prev)]
    ctx.in_grad_accumulate = list(accs)
    op.backward(ctx)
    for i, (got, p, x) in enumerate(zip(ctx.in_grads, prev, vals)):
        if i != drop:
            torch.testing.assert_close(got, x.grad + (p if accs[i] else 0), rtol=0, atol=1e-5, msg=f"input {i}")


def test_multihead_attention_trains_like_torch():
    from flexmi.core import LossType, SGDOptimizer
    B, T, E, H = 4, 6, 16, 4
    m = _cpu_model(B)
    x = m.create_tensor([B, T, E])
    m.dense(m.multihead_attention(x, x, x, E, H, causal=True, name="mha"), 1)
    assert [op.name for op in m.layers[:5]] == ["mha_q", "mha_k", "mha_v", "mha", "mha_o"]
    m.compile(SGDOptimizer(m, 0.05), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
    ex = m.init_layers()
    ws = [torch.from_numpy(p.get_weights(m).copy()) for p in m.parameters]    # q, k, v, o, head: weight, bias
    ref = torch.nn.MultiheadAttention(E, H, batch_first=True)
    head = torch.nn.Linear(E, 1)
    with torch.no_grad():                                # the mapping of the builder's docstring
        ref.in_proj_weight.copy_(torch.cat([ws[0], ws[2], ws[4]]))
        ref.in_proj_bias.copy_(torch.cat([ws[1], ws[3], ws[5]]))
        for dst, src in zip((ref.out_proj.weight, ref.out_proj.bias, head.weight, head.bias), ws[6:]):
            dst.copy_(src)
    opt = torch.optim.SGD(list(ref.parameters()) + list(head.parameters()), 0.05)
    rng = np.random.RandomState(1)
    hidden = torch.ones(T, T, dtype=torch.bool).triu(1)
    for _ in range(3):
        xv, lab = rng.randn(B, T, E).astype(np.float32), rng.randn(B, T, 1).astype(np.float32)
        ex.scatter_from_host(x, xv)
        ex.scatter_from_host(m.get_label_tensor(), lab)
        ex.train_step()
        opt.zero_grad()
        xt = torch.from_numpy(xv)
        (0.5 * (head(ref(xt, xt, xt, attn_mask=hidden, need_weights=False)[0]) - torch.from_numpy(lab)).pow(2).sum() / B).backward()
        opt.step()
    want = list(ref.in_proj_weight.detach().split(E)) + [ref.out_proj.weight.detach(), head.weight.detach()]
    for p, w, w0 in zip([m.parameters[i] for i in (0, 2, 4, 6, 8)], want, [ws[i] for i in (0, 2, 4, 6, 8)]):
        got = p.get_weights(m)
        assert np.abs(got - w.numpy()).max() / np.abs(w.numpy()).max() < 1e-5, p.name
        assert np.abs(got - w0.numpy()).max() > 1e-4, p.name                       # it trained


def test_limits_are_refused():
    from flexmi.core import LossType, SGDOptimizer
    with pytest.raises(ValueError, match="causal needs Tq == Tk"):
        m = _cpu_model(2)
        m.attention(m.create_tensor([2, 4, 8]), m.create_tensor([2, 5, 8]), m.create_tensor([2, 5, 8]), 2, causal=True)
    for device in ("cpu", "gpu"):
        m = _cpu_model(2, device)
        x = m.create_tensor([2, 4, 96])
        m.multihead_attention(x, x, x, 96, 2)            # dh = 48
        if device == "cpu":
            m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
        else:
            with pytest.raises(ValueError, match="Attention .* head dimension 48"):
                m.compile(SGDOptimizer(m, 0.1), LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE, [])
