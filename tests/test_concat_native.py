"""Native channel concat in training (K19, ``ops/csrc/concat.hip``) on the GPU.

Every comparison is bit equality: the kernels copy, select and add exactly as the torch path they
replace (``torch.cat``; ``torch.split`` + ``relu_backward``; chained ``a + b``), so no tolerance is
needed.  ``bigdl.deterministic`` is on wherever weight gradients are compared, so that split-K atomic
order does not decide.  The module tests run a twin with ``bigdl.concat.train=false`` (the parent
path) as the reference, and make ``torch.cat`` / ``torch.split`` raise on device tensors during the
second step of the run under test."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
_3A = ((64,), (96, 128), (16, 32), (32,))


@pytest.fixture(autouse=True)
def _setup():
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    config.set_property("bigdl.compute.dtype", "bf16")
    Engine.init(device="cuda:0")
    Engine.set_compute_dtype("bf16")
    config.set_property("bigdl.deterministic", True)
    from bigdl import ops
    assert ops.native_status()["loaded"]
    yield
    config.clear_property("bigdl.concat.train")
    config.set_property("bigdl.deterministic", False)
    config.set_property("bigdl.compute.dtype", "auto")
    Engine.set_compute_dtype("bf16")


def _NO():
    from bigdl.ops import native_ops
    return native_ops


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def _flat(t):
    """The tensor's memory as a 1-D view (NHWC order for a channels-last 4-D tensor)."""
    return t.permute(0, 2, 3, 1).view(-1) if t.dim() == 4 else t.view(-1)


def _rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return _cl(torch.randn(*shape, generator=g).to(dtype).to(dev))


class _NoTorchCat:
    """``torch.cat`` / ``torch.split`` raise on device tensors while active."""

    def __enter__(self):
        self.saved = [(torch, "cat", torch.cat), (torch, "concat", torch.concat), (torch, "split", torch.split)]

        def guard(name, fn):
            def g(first, *a, **k):
                ts = [first] if isinstance(first, torch.Tensor) else list(first)
                if any(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
                    raise AssertionError(f"torch.{name} called on a device tensor in the training step")
                return fn(first, *a, **k)
            return g
        for mod, name, fn in self.saved:
            setattr(mod, name, guard(name, fn))
        return self

    def __exit__(self, *exc):
        for mod, name, fn in self.saved:
            setattr(mod, name, fn)


class _Count:
    """Counts calls of one ``native_ops`` wrapper while active."""

    def __init__(self, name):
        self.name, self.n = name, 0

    def __enter__(self):
        NO = _NO()
        self.fn = getattr(NO, self.name)

        def f(*a, **k):
            self.n += 1
            return self.fn(*a, **k)
        setattr(NO, self.name, f)
        return self

    def __exit__(self, *exc):
        setattr(_NO(), self.name, self.fn)


# ------------------------------------------------------------------------------------------- kernels
# M = 30 rows with an odd chunk count per row (one ragged block); 396 rows (several blocks); 80000 rows
# (more chunks than the capped grid has threads: the grid-stride loop wraps)
_SHAPES = [(2, 3, 5), (4, 9, 11), (8, 100, 100)]
_PARTS = {torch.bfloat16: [8, 24, 16, 8], torch.float32: [4, 12, 8, 4]}


def _part_sets(dtype):
    w = 8 if dtype == torch.bfloat16 else 4
    return [_PARTS[dtype], [2 * w], [w] * 9]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_concat_forward_vs_torch(dtype):
    NO = _NO()
    for n, h, w in _SHAPES:
        for sizes in (_part_sets(dtype) if n == 2 else [_PARTS[dtype]]):
            xs = [_rand((n, c, h, w), dtype, i) for i, c in enumerate(sizes)]
            y = NO.concat_forward(xs[0], xs[1:])
            assert y is not NotImplemented
            assert y.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(y, torch.cat(xs, 1))
    x2 = [_rand((5, c), dtype, i) for i, c in enumerate((16, 8, 8))]
    y2 = NO.concat_forward(x2[0], x2[1:])
    assert y2 is not NotImplemented and y2.is_contiguous() and torch.equal(y2, torch.cat(x2, 1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_concat_split_backward_vs_torch(dtype):
    NO = _NO()
    zero = torch.zeros((), dtype=dtype, device=dev)

    def check(shape, sizes, masks):
        C = sum(sizes)
        y = _rand((shape[0], C) + shape[1:], dtype, 7)     # negatives under every part, the unmasked too
        _flat(y)[::3] = 0                                 # exact zeros
        _flat(y)[1::11] = -0.0
        gy = _rand((shape[0], C) + shape[1:], dtype, 8)
        got = NO.concat_split_backward(gy, y, sizes, masks)
        assert got is not NotImplemented and len(got) == len(sizes)
        c0 = 0
        for g, c, m in zip(got, sizes, masks):
            gk, yk = gy[:, c0:c0 + c], y[:, c0:c0 + c]
            want = torch.where(yk > 0, gk, zero) if m else gk
            assert g.shape == want.shape
            assert g.is_contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g.is_contiguous()
            assert torch.equal(g, want)
            if m:  # the bits of the ReLU backward it replaces
                assert torch.equal(g, NO.relu_backward(_cl(gk), _cl(yk), 0.0))
            c0 += c

    for n, h, w in _SHAPES:
        check((n, h, w), _PARTS[dtype], [True, False, True, True])
    one, nine = _part_sets(dtype)[1:]
    check((2, 3, 5), one, [True])
    check((2, 3, 5), nine, [True, False, True] * 3)
    check((5,), [16, 8, 8], [False, True, True])
    # no masked part: y is not needed
    gy = _rand((2, sum(_PARTS[dtype]), 3, 5), dtype, 9)
    plain = NO.concat_split_backward(gy, None, _PARTS[dtype])
    assert all(torch.equal(a, b) for a, b in zip(plain, torch.split(gy, _PARTS[dtype], 1)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_sum_n_vs_left_to_right_torch_sum(dtype, k):
    NO = _NO()
    for shape in [(2, 16, 3, 5), (1003,), (8, 64, 100, 100)]:   # vector body, scalar tail, grid-stride wrap
        ts = [_rand(shape, dtype, 20 + i) for i in range(k)]
        # where one rounding and a rounding per add differ: 1 + 2^-9 + 2^-9 and the tie 1 + 2^-8 + 2^-8
        # (bf16), 1 + 2^-24 + 2^-24 (fp32)
        _flat(ts[0])[:3] = 1.0
        for t in ts[1:]:
            _flat(t)[:3] = 0.0
        tiny = [2.0 ** -9, 2.0 ** -8, 2.0 ** -24]
        for t in ts[1:3]:
            _flat(t)[:3] = torch.tensor(tiny, dtype=dtype, device=dev)
        want = ts[0]
        for t in ts[1:]:
            want = want + t
        got = NO.sum_n(ts[0], ts[1:])
        assert got is not NotImplemented and got.stride() == ts[0].stride()
        assert torch.equal(got, want)
        if k >= 3 and dtype == torch.bfloat16:
            assert _flat(got)[1].item() == 1.0   # a single rounding would give 1.0078125


def test_unaligned_part_is_not_implemented_and_module_uses_torch():
    from bigdl import ops
    from bigdl.nn import JoinTable
    from bigdl.utils.table import Table
    NO = _NO()
    a, b = _rand((2, 8, 3, 5), torch.bfloat16, 1), _rand((2, 6, 3, 5), torch.bfloat16, 2)
    gy = _rand((2, 14, 3, 5), torch.bfloat16, 3)
    assert NO.concat_forward(a, [b]) is NotImplemented
    assert NO.concat_split_backward(gy, None, [8, 6]) is NotImplemented
    assert NO.concat_forward(a, [a.float()]) is NotImplemented          # dtypes differ
    odd = torch.empty(5 * 16 + 8, dtype=torch.bfloat16, device=dev)[1:81].view(5, 16)   # a 2-byte-aligned pointer
    assert odd.is_contiguous() and NO.concat_forward(odd, [odd]) is NotImplemented
    assert NO.sum_n(odd, [odd, odd]) is NotImplemented
    assert NO.sum_n(a, [a, a.float()]) is NotImplemented
    j = JoinTable(2, 0)
    j.training()
    y = j.forward(Table(a, b))
    assert torch.equal(y, torch.cat([a, b], 1))
    gi = j.backward(Table(a, b), gy)
    assert torch.equal(gi[1], gy[:, :8]) and torch.equal(gi[2], gy[:, 8:])
    ops.reset_fallbacks()


# ------------------------------------------------------------------------------------------- modules
def _param_grads(m):
    _, gs = m.parameters()
    return [g.clone() for g in gs]


def _two_steps(m, x, gy, guard):
    """Two training passes of a module (the first records the concat shapes); the second one
    optionally under the torch.cat / torch.split guard.  Returns (output, gradInput, parameter grads)."""
    for step in range(2):
        m.zeroGradParameters()
        if guard and step == 1:
            with _NoTorchCat():
                y = m.forward(x)
                gi = m.backward(x, gy)
        else:
            y = m.forward(x)
            gi = m.backward(x, gy)
    torch.cuda.synchronize()
    return y.clone(), gi.clone(), _param_grads(m)


def _run_on_off(build, x, gy, check_on=None):
    from bigdl.utils import config
    from bigdl.nn.fusion import fuse
    m_on = build()
    m_off = copy.deepcopy(m_on)
    res = []
    for m, on in ((m_on, True), (m_off, False)):
        config.set_property("bigdl.concat.train", on)
        m.cuda()
        m.training()
        fuse(m)
        res.append(_two_steps(m, x, gy, guard=on))
        if on and check_on is not None:
            check_on(m)
    (y1, g1, p1), (y0, g0, p0) = res
    assert y1.dtype == y0.dtype and torch.equal(y1, y0), "output differs from the torch path"
    assert torch.equal(g1, g0), "gradInput differs from the torch path"
    assert len(p1) == len(p0) and all(torch.equal(a, b) for a, b in zip(p1, p0)), "a parameter gradient differs"
    return m_on


def _mask_flags_clear(m):
    from bigdl.nn.layers.activation import Threshold
    assert not any("_premasked" in t.__dict__ for t in m.flattened_modules() if isinstance(t, Threshold))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_v1_block_concat_form(mode):
    from bigdl.models.inception import Inception_Layer_v1
    from bigdl.nn.containers import _final_conv
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    dtype = torch.bfloat16 if mode == "bf16" else torch.float32
    config.set_property("bigdl.compute.dtype", mode)
    Engine.set_compute_dtype(mode)
    x = _rand((2, 192, 8, 8), dtype, 1)
    gy = _rand((2, 256, 8, 8), dtype, 2)

    def check_on(m):
        _mask_flags_clear(m)
        if mode != "bf16":
            return  # fp32 compute: fused backward, no zero-copy forward
        c0 = 0
        for br in m.modules:  # every branch's final conv wrote its slice of the block output
            conv = _final_conv(br)
            assert conv.output.data_ptr() == m.output.data_ptr() + c0 * m.output.element_size()
            c0 += conv.nOutputPlane
        assert c0 == m.output.shape[1]

    with _Count("concat_split_backward") as split, _Count("sum_n") as sums:
        _run_on_off(lambda: Inception_Layer_v1(192, _3A, "b/"), x, gy, check_on)
    assert split.n == 2 and sums.n == 2   # once per backward of the run under test, none in the twin


def test_v1_blocks_graph_form():
    from bigdl.models.inception import _v1_node
    from bigdl.nn import Graph, Input
    from bigdl.nn.layers.table_ops import JoinTable
    x = _rand((2, 192, 8, 8), torch.bfloat16, 1)
    gy = _rand((2, 480, 8, 8), torch.bfloat16, 2)

    def build():
        inp = Input()
        return Graph(inp, _v1_node(_v1_node(inp, "3a"), "3b"))

    def check_on(g):
        _mask_flags_clear(g)
        joins = [n for n in g.forward_order if isinstance(n.element, JoinTable)]
        assert len(joins) == 2
        for n in joins:  # the join's inputs are the consecutive channel slices of its output
            y, c0 = n.element.output, 0
            for p in n.prev_nodes:
                assert p.element.output.data_ptr() == y.data_ptr() + c0 * y.element_size()
                c0 += p.element.output.shape[1]
            assert c0 == y.shape[1]

    with _Count("concat_split_backward") as split, _Count("sum_n") as sums:
        _run_on_off(build, x, gy, check_on)
    assert split.n == 4      # two joins, two backwards
    assert sums.n == 4       # the four consumers of each block input, summed when the node's turn comes


def test_unplannable_join_with_bare_pooling_branch():
    from bigdl.nn import Concat, ReLU, Sequential, SpatialConvolution, SpatialMaxPooling
    x = _rand((2, 64, 8, 8), torch.bfloat16, 1)
    gy = _rand((2, 32 + 48 + 64, 8, 8), torch.bfloat16, 2)

    def build():
        cat = Concat(2)
        cat.add(Sequential(SpatialConvolution(64, 32, 1, 1), ReLU(True)))
        cat.add(Sequential(SpatialConvolution(64, 16, 1, 1), ReLU(True),
                           SpatialConvolution(16, 48, 3, 3, 1, 1, 1, 1), ReLU(True)))
        cat.add(Sequential(SpatialMaxPooling(3, 3, 1, 1, 1, 1).ceil()))
        return cat

    seen = []

    def check_on(m):
        _mask_flags_clear(m)
        assert m._plan is not None and m._plan.convs[2] is None and m._plan.arm((2, 64, 8, 8), x, True) is None

    NO = _NO()
    real = NO.concat_split_backward

    def spy(gy_, y_, sizes, masks=None):
        seen.append(list(masks))
        return real(gy_, y_, sizes, masks)
    NO.concat_split_backward = spy
    try:
        with _Count("concat_forward") as fwd:
            _run_on_off(build, x, gy, check_on)
    finally:
        NO.concat_split_backward = real
    assert fwd.n == 2                                   # both forwards of the run under test
    assert seen == [[True, True, False]] * 2            # the pooling branch's part is not masked


def test_whole_model_two_sgd_steps():
    from bigdl.dataset import MiniBatch
    from bigdl.models.inception import Inception_v1_NoAuxClassifier
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim import SGD
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.utils import config
    m_on = Inception_v1_NoAuxClassifier(1000, has_dropout=False)
    m_off = copy.deepcopy(m_on)
    x = _rand((2, 3, 224, 224), torch.bfloat16, 1)
    t = torch.tensor([3.0, 700.0], device=dev)
    res = []
    for m, on in ((m_on, True), (m_off, False)):
        config.set_property("bigdl.concat.train", on)
        opt = LocalOptimizer(m, [MiniBatch(x, t)], ClassNLLCriterion(),
                             SGD(learningrate=0.01, momentum=0.9, dampening=0.0, weightdecay=1e-4), batch_size=2)
        opt.prepare()
        l0 = opt.train_step(MiniBatch(x, t)).clone()
        if on:
            with _NoTorchCat():
                l1 = opt.train_step(MiniBatch(x, t)).clone()
        else:
            l1 = opt.train_step(MiniBatch(x, t)).clone()
        torch.cuda.synchronize()
        res.append((l0, l1, opt.flat.weight.clone()))
    (a0, a1, wa), (b0, b1, wb) = res
    assert bool(torch.isfinite(a1).all())
    assert torch.equal(a0, b0) and torch.equal(a1, b1), "loss differs from the torch path"
    assert torch.equal(wa, wb), "weights differ from the torch path after two steps"
