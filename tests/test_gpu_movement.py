"""Concat / split / copy on the HIP multi-copy kernel (``fm_multi_copy``) through
``flexmi.ops._kernels``, fp32 and bf16: 16-B vector pieces (inner sizes that are multiples of 8 at
aligned offsets), scalar pieces (odd inner sizes), both in one call, a piece whose destination
offset breaks 16-B alignment, axis 0 / middle / last of a 3-D tensor, per-piece accumulate flags,
``None`` gradients, and more than 32 pieces (the mask of one launch table).  Expected values are
exact (``torch.equal``): copies are bit-identical, fp32 accumulation is ``a + b``, bf16 accumulation
is ``(a.float() + b.float()).bfloat16()`` -- the kernel adds in fp32 and rounds once, to nearest even.
tests/test_movement_masks_cpu.py runs the same cases against a torch emulation of the descriptors."""
from types import SimpleNamespace

import pytest
import torch

from flexmi.ops import _kernels as Kk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _rand(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dt).cuda()


def _add(a, b):
    """dst (+)= src as the kernel computes it: one fp32 add, rounded once to the tensor's type."""
    return (a.float() + b.float()).to(a.dtype)


def _shape(s, axis):
    d = [3, 5]
    d.insert(axis, s)
    return tuple(d)


# sizes along the axis: 16-B-able pieces, odd pieces, both mixed (every offset after the 3 is odd), and a
# total that allows 16-B rows with a piece (the third) whose offset does not
SIZES = {"vec": [8, 16, 24], "odd": [3, 5, 7], "mixed": [8, 3, 16, 5], "misaligned": [8, 2, 8, 6]}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("kind", sorted(SIZES))
def test_concat_split_forward_backward(gpu, dt, axis, kind):
    sizes = SIZES[kind]
    xs = [_rand(_shape(s, axis), dt, 10 + i) for i, s in enumerate(sizes)]
    full = torch.cat(xs, axis)
    y = torch.full_like(full, 7.0)
    Kk.concat_forward(xs, y, axis)
    assert torch.equal(y, full)
    outs = [torch.full_like(x, 7.0) for x in xs]
    Kk.split_forward(full, outs, axis)
    for o, x in zip(outs, xs):
        assert torch.equal(o, x)
    # concat backward: alternate accumulating / overwriting gradients
    accs = [i % 2 == 0 for i in range(len(xs))]
    g0 = [_rand(x.shape, dt, 50 + i) for i, x in enumerate(xs)]
    gs = [g.clone() for g in g0]
    Kk.concat_backward(full, gs, accs, axis)
    for g, b, x, a in zip(gs, g0, xs, accs):
        assert torch.equal(g, _add(b, x) if a else x)
    # split backward: dx (+)= cat(out_grads)
    for acc in (False, True):
        dx0 = _rand(full.shape, dt, 90)
        dx = dx0.clone()
        Kk.split_backward(xs, dx, acc, axis)
        assert torch.equal(dx, _add(dx0, full) if acc else full)


@pytest.mark.parametrize("dt", DTYPES)
def test_concat_backward_acc_flags_and_none(gpu, dt):
    axis = 1
    xs = [_rand(_shape(s, axis), dt, i) for i, s in enumerate([5, 8, 3])]
    dy = torch.cat(xs, axis)
    g0 = [_rand(x.shape, dt, 20 + i) for i, x in enumerate(xs)]
    gs = [g.clone() for g in g0]
    Kk.concat_backward(dy, gs, [True, False, True], axis)
    assert torch.equal(gs[0], _add(g0[0], xs[0]))
    assert torch.equal(gs[1], xs[1])
    assert torch.equal(gs[2], _add(g0[2], xs[2]))
    # a gradient-less input in the middle: the later slice starts after it, and keeps ITS flag
    for accs in ([False, True, True], [True, True, False]):
        gs = [g0[0].clone(), None, g0[2].clone()]
        Kk.concat_backward(dy, gs, accs, axis, [tuple(x.shape) for x in xs])
        assert torch.equal(gs[0], _add(g0[0], xs[0]) if accs[0] else xs[0])
        assert torch.equal(gs[2], _add(g0[2], xs[2]) if accs[2] else xs[2])
    with pytest.raises(AssertionError):
        Kk.concat_backward(dy, [g0[0].clone(), None, g0[2].clone()], [False] * 3, axis)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("none_at", [0, 1, 2])
def test_split_backward_none_accumulates(gpu, dt, none_at):
    """The split's input has another consumer: dx already holds its gradient, every present piece
    must ADD (on the parent commit a leading None shifted the mask and the first piece overwrote)."""
    axis = 1
    gs = [_rand(_shape(s, axis), dt, i) for i, s in enumerate([8, 5, 3])]
    shapes = [tuple(g.shape) for g in gs]
    ogs = [None if i == none_at else g for i, g in enumerate(gs)]
    dx0 = _rand(_shape(16, axis), dt, 40)
    dx = dx0.clone()
    Kk.split_backward(ogs, dx, True, axis, shapes)
    inc = torch.cat([torch.zeros_like(g) if o is None else g for g, o in zip(gs, ogs)], axis)
    assert torch.equal(dx, _add(dx0, inc))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("none_at", [0, 1, 2])
def test_split_op_backward_unused_output(gpu, dt, none_at):
    """Split.backward with acc=False and an unused output: dx is zeroed, then the pieces add."""
    from flexmi.ops.tensor_ops import Split
    axis = 2
    gs = [_rand(_shape(s, axis), dt, i) for i, s in enumerate([3, 8, 5])]
    ogs = [None if i == none_at else g for i, g in enumerate(gs)]
    dx = _rand(_shape(16, axis), dt, 41)
    ctx = SimpleNamespace(in_grads=[dx], out_grads=ogs, in_grad_accumulate=[False], hip=True, outputs=gs)
    Split.backward(SimpleNamespace(axis=axis), ctx)
    assert torch.equal(dx, torch.cat([torch.zeros_like(g) if o is None else g for g, o in zip(gs, ogs)], axis))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 1001])
def test_copy_or_add(gpu, dt, n):
    src, dst0 = _rand((n,), dt, 1), _rand((n,), dt, 2)
    dst = dst0.clone()
    Kk.copy_or_add(src, dst, False)
    assert torch.equal(dst, src)
    dst = dst0.clone()
    Kk.copy_or_add(src, dst, True)
    assert torch.equal(dst, _add(dst0, src))


@pytest.mark.parametrize("dt", DTYPES)
def test_more_than_32_pieces(gpu, dt):
    """40-input concat and its backward with alternating flags (accumulating pieces at index >= 32),
    and a 35-way split backward that accumulates: every flag must reach its piece."""
    axis = 1
    sizes = [1 + (i * 3) % 4 for i in range(40)]
    xs = [_rand(_shape(s, axis), dt, i) for i, s in enumerate(sizes)]
    full = torch.cat(xs, axis)
    y = torch.full_like(full, 7.0)
    Kk.concat_forward(xs, y, axis)
    assert torch.equal(y, full)
    accs = [i % 2 == 1 for i in range(40)]
    g0 = [_rand(x.shape, dt, 100 + i) for i, x in enumerate(xs)]
    gs = [g.clone() for g in g0]
    Kk.concat_backward(full, gs, accs, axis)
    for i, (g, b, x, a) in enumerate(zip(gs, g0, xs, accs)):
        assert torch.equal(g, _add(b, x) if a else x), i
    part = torch.cat(xs[:35], axis)
    dx0 = _rand(part.shape, dt, 300)
    dx = dx0.clone()
    Kk.split_backward(xs[:35], dx, True, axis)
    assert torch.equal(dx, _add(dx0, part))
    # with the second piece unused
    dx = dx0.clone()
    Kk.split_backward([xs[0], None] + xs[2:35], dx, True, axis, [tuple(x.shape) for x in xs[:35]])
    inc = torch.cat([xs[0], torch.zeros_like(xs[1])] + xs[2:35], axis)
    assert torch.equal(dx, _add(dx0, inc))


def test_binding_refuses_flags_beyond_its_mask(gpu):
    """More accumulating pieces than the 32-bit mask of one call carries: an error, not dropped bits."""
    t = [torch.zeros(4, device=gpu) for _ in range(33)]
    z, one, four = [0] * 33, [1] * 33, [4] * 33
    with pytest.raises(RuntimeError, match="multi_copy"):
        Kk.C().multi_copy(t, z, t, z, one, four, four, four, 1)
    with pytest.raises(RuntimeError, match="multi_copy"):
        Kk.C().multi_copy(t[:2], z[:2], t[:2], z[:2], one[:2], four[:2], four[:2], four[:2], 4)
    src = [torch.full((4,), float(i), device=gpu) for i in range(33)]
    Kk.C().multi_copy(src, z, t, z, one, four, four, four, 0)       # pure copies may exceed 32
    assert torch.equal(torch.stack(t), torch.stack(src))
