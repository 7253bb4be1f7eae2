"""Channel concat in training (K19) without a GPU: the torch twins of the three concat ops, and the
module layer's guarantees — the CPU path is bit-for-bit the torch path whatever ``bigdl.concat.train`` says,
the one-shot "gradient already masked" flag of a mask-``Threshold`` never outlives the backward that
set it, and eval mode keeps the inference ConcatPlan behaviour."""
import copy

import pytest
import torch

from bigdl.ops import reference as R
from bigdl.utils import config

_3A = ((64,), (96, 128), (16, 32), (32,))


@pytest.fixture(autouse=True)
def _props():
    yield
    config.clear_property("bigdl.concat.train")


def _block():
    from bigdl.models.inception import Inception_Layer_v1
    from bigdl.nn.fusion import fuse
    m = Inception_Layer_v1(192, _3A, "b/")
    m.training()
    fuse(m)
    return m


def _grads(m):
    _, gs = m.parameters()
    return [g.clone() for g in gs]


# ------------------------------------------------------------------------------------------- reference ops
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_concat_forward(dtype):
    xs = [torch.randn(2, c, 3, 5).to(dtype) for c in (8, 24, 16, 8)]
    assert torch.equal(R.concat_forward(xs[0], xs[1:]), torch.cat(xs, 1))
    assert torch.equal(R.concat_forward(xs[0]), xs[0])
    x2 = [torch.randn(5, c).to(dtype) for c in (16, 8, 8)]
    assert torch.equal(R.concat_forward(x2[0], x2[1:]), torch.cat(x2, 1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_concat_split_backward(dtype):
    sizes, masks = [8, 24, 16, 8], [True, False, True, True]
    y = torch.randn(2, 56, 3, 5).to(dtype)
    y[:, ::3] = 0  # exact zeros: masked out
    gy = torch.randn(2, 56, 3, 5).to(dtype)
    got = R.concat_split_backward(gy, y, sizes, masks)
    c0 = 0
    for g, c, m in zip(got, sizes, masks):
        gk, yk = gy[:, c0:c0 + c], y[:, c0:c0 + c]
        want = torch.where(yk > 0, gk, torch.zeros((), dtype=dtype)) if m else gk
        assert g.is_contiguous() and torch.equal(g, want)
        if m:  # the bits of the ReLU backward it replaces
            assert torch.equal(g, R.relu_backward(gk.contiguous(), yk.contiguous(), 0.0))
        c0 += c
    plain = R.concat_split_backward(gy, None, sizes)
    assert all(torch.equal(a, b) for a, b in zip(plain, torch.split(gy, sizes, 1)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_reference_sum_n(dtype, k):
    ts = [torch.randn(2, 16, 3, 5).to(dtype) for _ in range(k)]
    want = ts[0]
    for t in ts[1:]:
        want = want + t
    assert torch.equal(R.sum_n(ts[0], ts[1:]), want)


def test_dispatcher_routes_host_tensors_to_the_reference():
    from bigdl import ops
    xs = [torch.randn(2, c, 3, 5) for c in (8, 6)]
    y = ops.concat_forward(xs[0], xs[1:])
    assert torch.equal(y, torch.cat(xs, 1))
    gs = ops.concat_split_backward(torch.ones_like(y), y, [8, 6], [True, False])
    assert torch.equal(gs[0], (xs[0] > 0).float()) and torch.equal(gs[1], torch.ones_like(xs[1]))
    assert torch.equal(ops.sum_n(xs[0], [xs[0], xs[0]]), xs[0] + xs[0] + xs[0])
    assert ops.fallback_counts() == {}


def test_reference_sum_n_rounds_after_every_add():
    a = torch.tensor([1.0], dtype=torch.bfloat16)
    e = torch.tensor([2.0 ** -9], dtype=torch.bfloat16)
    assert R.sum_n(a, [e, e]).item() == ((a + e) + e).item() == 1.0
    # bf16 spacing at 1 is 2^-7: 1 + 2^-8 is a tie and rounds to even (1), twice; one rounding of the
    # fp32 sum 1 + 2^-7 would keep it
    h = torch.tensor([2.0 ** -8], dtype=torch.bfloat16)
    assert R.sum_n(a, [h, h]).item() == 1.0
    assert (a.float() + h.float() + h.float()).to(torch.bfloat16).item() == 1.0078125


# ------------------------------------------------------------------------------------------- module layer
def test_v1_block_cpu_same_bits_on_and_off():
    m_on = _block()
    m_off = copy.deepcopy(m_on)
    x = torch.randn(2, 192, 8, 8)
    gy = torch.randn(2, 256, 8, 8)
    res = []
    for m, on in ((m_on, True), (m_off, False)):
        config.set_property("bigdl.concat.train", on)
        for _ in range(2):
            m.zeroGradParameters()
            y = m.forward(x)
            gi = m.backward(x, gy)
        res.append((y.clone(), gi.clone(), _grads(m)))
    (y1, g1, p1), (y0, g0, p0) = res
    assert torch.equal(y1, y0) and torch.equal(g1, g0)
    assert all(torch.equal(a, b) for a, b in zip(p1, p0))


def _mask_thresholds(m):
    from bigdl.nn.layers.activation import Threshold
    return [t for t in m.flattened_layers() if isinstance(t, Threshold) and t._passthrough == "mask"]


def test_flag_not_left_behind_and_backward_twice():
    m = _block()
    ths = _mask_thresholds(m)
    assert len(ths) == 6
    x = torch.randn(2, 192, 8, 8)
    gy = torch.randn(2, 256, 8, 8)
    m.forward(x)
    g1 = m.backward(x, gy).clone()
    assert not any("_premasked" in t.__dict__ for t in ths)
    g2 = m.backward(x, gy).clone()
    assert torch.equal(g1, g2)
    assert not any("_premasked" in t.__dict__ for t in ths)


def test_update_grad_input_plus_acc_equals_backward():
    m1 = _block()
    m2 = copy.deepcopy(m1)
    x = torch.randn(2, 192, 8, 8)
    gy = torch.randn(2, 256, 8, 8)
    for m in (m1, m2):
        m.zeroGradParameters()
        m.forward(x)
    ga = m1.backward(x, gy)
    gb = m2.updateGradInput(x, gy)
    m2.accGradParameters(x, gy)
    assert torch.equal(ga, gb)
    assert all(torch.equal(a, b) for a, b in zip(_grads(m1), _grads(m2)))
    assert not any("_premasked" in t.__dict__ for t in _mask_thresholds(m2))


def test_threshold_flag_is_one_shot():
    """A mask-Threshold outside any join masks as always; a flag set on it passes exactly one
    gradient through and is gone."""
    from bigdl.nn import ReLU, Sequential, SpatialConvolution
    from bigdl.nn.fusion import fuse
    s = Sequential(SpatialConvolution(8, 8, 1, 1), ReLU(True))
    s.training()
    fuse(s)
    th = s.modules[1]
    assert th._passthrough == "mask"
    x = torch.randn(2, 8, 4, 4)
    y = s.forward(x)
    g = torch.randn_like(y)
    want = R.relu_backward(g, y, 0.0)
    assert torch.equal(th.updateGradInput(y, g), want)
    th._premasked = True
    assert th.updateGradInput(y, g) is g
    assert "_premasked" not in th.__dict__
    assert torch.equal(th.updateGradInput(y, g), want)
    s.backward(x, g)
    assert torch.equal(th.gradInput, want)


def test_graph_fanout_sum_keeps_bits_and_order():
    """Four consumers of one node: the deferred gradient sum equals the chained adds in arrival order."""
    from bigdl.nn import CAddTable, Graph, Input, Linear
    inp = Input()
    ls = [Linear(6, 6)(inp) for _ in range(4)]
    g = Graph(inp, CAddTable()(*ls))
    x = torch.randn(3, 6)
    go = torch.randn(3, 6)
    g.forward(x)
    gi = g.backward(x, go)
    # backward visits the consumers in reverse forward order and adds as they arrive
    want = None
    for n in reversed(ls):
        d = n.element.gradInput
        want = d if want is None else want + d
    assert torch.equal(gi, want)


def test_eval_mode_and_inference_plan_unchanged():
    from bigdl.nn.containers import ConcatPlan
    m = _block()
    x = torch.randn(2, 192, 8, 8)
    y_train = m.forward(x).clone()
    m.evaluate()
    outs = [b.forward(x) for b in m.modules]
    y = m.forward(x)
    assert torch.equal(y, torch.cat(outs, 1)) and torch.equal(y, y_train)
    # the plan exists, records device shapes only, and never arms for a host tensor
    assert isinstance(m._plan, ConcatPlan) and m._plan.shapes == {}
    assert all(c is not None for c in m._plan.convs)
    assert m._plan.arm((2, 192, 8, 8), x) is None and m._plan.arm((2, 192, 8, 8), x, True) is None
    assert all(c._out_target is None for c in m._plan.convs)
