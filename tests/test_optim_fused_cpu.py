"""Host side of the fused updates of the elementwise methods: the torch forms stay the CPU path (and
the oracle of the kernels in tests/test_optim_fused.py), accept the bf16 wire gradient shard, and
``bigdl.optim.fused`` never changes what runs on the CPU."""
import pickle

import pytest
import torch

N = 203
SCALE = 1.0 / 3  # not a power of two: a product formed in bf16 would round


def _methods():
    from bigdl import optim as O
    return {"rmsprop": lambda: O.RMSprop(learningrate=0.01, learningrate_decay=0.001, decayrate=0.99, epsilon=1e-8),
            "adadelta": lambda: O.Adadelta(decayrate=0.9, epsilon=1e-6),
            "adamax": lambda: O.Adamax(),
            "ftrl": lambda: O.Ftrl(learningrate=0.05, initial_accumulator_value=0.1, l1_regularization_strength=1e-2,
                                   l2_regularization_strength=1e-3, l2_shrinkage_regularization_strength=1e-4),
            "adam": lambda: O.Adam(learningrate=0.01, learningrate_decay=0.001),
            "adagrad": lambda: O.Adagrad(learningrate=0.01, learningrate_decay=0.001, weightdecay=1e-3)}


NAMES = ["rmsprop", "adadelta", "adamax", "ftrl", "adam", "adagrad"]


def _run(name, grads, steps):
    """``steps`` sliced updates of a seeded CPU vector; returns the weights, shadow and state tensors."""
    meth = _methods()[name]()
    meth.grad_scale = SCALE
    x = torch.randn(N, generator=torch.Generator().manual_seed(2))
    shadow = torch.zeros(N, dtype=torch.bfloat16)
    for i in range(steps):
        meth.begin_iteration(x)
        meth.apply_update(x, grads[i], 0, N, shadow=shadow)
    states = {k: v.clone() for k, v in meth.state.items() if isinstance(v, torch.Tensor)}
    return x, shadow, states


def _grads(steps, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return [torch.randn(N, generator=g).to(dtype) for _ in range(steps)]


@pytest.mark.parametrize("name", NAMES)
def test_bf16_gradient_equals_widened_gradient_on_cpu(name):
    g16 = _grads(2, torch.bfloat16)
    x16, sh16, st16 = _run(name, g16, 2)
    x32, sh32, st32 = _run(name, [g.float() for g in g16], 2)
    assert x16.dtype == torch.float32 and torch.isfinite(x16).all()
    assert torch.equal(x16, x32) and torch.equal(sh16, sh32)
    assert st16.keys() == st32.keys() and len(st16) >= 1
    for k in st16:
        assert st16[k].dtype == torch.float32 and torch.equal(st16[k], st32[k]), k


def test_adam_reference_step_takes_a_bf16_gradient():
    from bigdl import ops
    g16 = _grads(1, torch.bfloat16)[0]
    outs = []
    for g in (g16, g16.float()):
        w = torch.randn(N, generator=torch.Generator().manual_seed(2))
        m, v = torch.zeros(N), torch.zeros(N)
        ops.adam_step(w, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1, 0.0, SCALE, None)
        outs.append((w, m, v))
    for a, b in zip(*outs):
        assert a.dtype == torch.float32 and torch.equal(a, b)


def test_property_default_and_bf16_flags():
    from bigdl.utils import config
    from bigdl import optim as O
    assert config.get_property("bigdl.optim.fused") is True
    for cls in (O.RMSprop, O.Adadelta, O.Adamax, O.Ftrl, O.Adam):
        assert cls.reads_bf16_grad is True, cls


@pytest.mark.parametrize("name", NAMES)
def test_property_never_changes_the_cpu_path(name):
    from bigdl.utils import config
    grads = _grads(3)
    try:
        config.set_property("bigdl.optim.fused", True)
        on = _run(name, grads, 3)
        config.set_property("bigdl.optim.fused", False)
        off = _run(name, grads, 3)
    finally:
        config.clear_property("bigdl.optim.fused")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k


def test_adam_pickled_before_a_step_reproduces_that_step():
    """State keys, ``evalCounter`` and the per-iteration scalars survive a pickle: an Adam saved after
    its first step and restored after the second was taken repeats the second step bit for bit."""
    grads = _grads(2)
    meth = _methods()["adam"]()
    meth.grad_scale = SCALE
    x = torch.randn(N, generator=torch.Generator().manual_seed(2))
    meth.optimize(lambda _x: (0.0, grads[0]), x)
    assert meth.state["evalCounter"] == 1 and {"s", "r"} <= set(meth.state)
    blob, x1 = pickle.dumps(meth), x.clone()
    meth.optimize(lambda _x: (0.0, grads[1]), x)
    assert meth.state["evalCounter"] == 2 and not torch.equal(x, x1)
    back = pickle.loads(blob)
    assert back.state["evalCounter"] == 1
    back.optimize(lambda _x: (0.0, grads[1]), x1)
    assert back.state["evalCounter"] == 2 and torch.equal(x1, x)
    for k in ("s", "r"):
        assert torch.equal(back.state[k], meth.state[k]), k
