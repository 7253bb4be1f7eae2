"""Gradient clipping as one object (bigdl.parameters.GradClip), host side: its torch form is the two
parameter processors bit for bit, the property that gates the fused path exists, CPU weights keep
the processor path with unchanged results, and the training CLIs wire the reference's three options."""
import contextlib
import copy

import pytest
import torch

from bigdl.parameters import ConstantClippingProcessor, L2NormClippingProcessor, run_processors

SCALE = 0.25
LO, HI = -0.3, 0.2


def _g_scaled(n=4099, seed=3):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    return g * SCALE


def _norm(g):
    return float(g.double().square().sum().sqrt())


def _settings():
    """name -> (threshold or None, clamp or None); thresholds relative to ‖g·scale‖ of ``_g_scaled()``."""
    n = _norm(_g_scaled())
    return {"clamp": (None, (LO, HI)), "l2_above": (0.5 * n, None), "l2_below": (2.0 * n, None),
            "both": (0.5 * n, (LO, HI))}


@pytest.mark.parametrize("setting", ["clamp", "l2_above", "l2_below", "both"])
def test_apply_is_the_processors_bit_for_bit(setting):
    from bigdl.parameters import GradClip
    thr, clamp = _settings()[setting]
    procs = []
    if clamp is not None:
        procs.append(ConstantClippingProcessor(*clamp))
    if thr is not None:
        procs.append(L2NormClippingProcessor(thr))
    want = _g_scaled()
    raw = want.clone()
    run_processors(procs, None, want)
    clip = GradClip.of(clamp, thr)
    got = _g_scaled()
    assert clip.apply(got) is got
    assert torch.equal(got, want)
    # the setting did what its name says
    assert torch.equal(want, raw) == (setting == "l2_below")
    assert [type(p) for p in clip.processors()] == [type(p) for p in procs]


def test_no_setting_is_no_object():
    from bigdl.parameters import GradClip
    assert GradClip.of(None, None) is None


def test_property_exists_and_defaults_to_true():
    from bigdl.utils import config
    assert config.get_property("bigdl.clip.fused") is True


@contextlib.contextmanager
def _cpu_engine():
    from bigdl.utils.engine import Engine
    old_dev, old_dt = Engine.device(), Engine.compute_dtype()
    Engine.set_device("cpu")
    Engine.set_compute_dtype("fp32")
    try:
        yield
    finally:
        Engine.set_device(old_dev)
        Engine.set_compute_dtype(old_dt)


def _mlp():
    from bigdl.nn import Sequential, Linear, Tanh, LogSoftMax
    from bigdl.utils.random import RNG
    RNG.setSeed(7)
    torch.manual_seed(7)
    return Sequential().add(Linear(16, 32)).add(Tanh()).add(Linear(32, 4)).add(LogSoftMax())


def _weights(model):
    return torch.cat([p.detach().reshape(-1).float().cpu() for p in model.parameters()[0]])


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_cpu_local_optimizer_keeps_the_processor_path(method, monkeypatch):
    """CPU weights: clipping goes through ``run_processors`` whatever ``bigdl.clip.fused`` says, and
    the weights are those of the update as it was before the fused path existed (the processors
    over the whole gradient, then the unclipped update), bit for bit."""
    import bigdl.parameters as P
    from bigdl import optim as O
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    make = {"sgd": lambda: O.SGD(learningrate=0.1, momentum=0.9, dampening=0.0),
            "adam": lambda: O.Adam(learningrate=0.01)}[method]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(8, 16, generator=gen) * 10
    y = (torch.randint(0, 4, (8,), generator=gen) + 1).float()
    calls = []
    real = P.run_processors

    def spy(procs, *a, **k):
        calls.append([type(p).__name__ for p in procs])
        return real(procs, *a, **k)
    monkeypatch.setattr(P, "run_processors", spy)
    with _cpu_engine():
        m1 = _mlp()
        m2 = copy.deepcopy(m1)
        w0 = _weights(m1)
        opt = LocalOptimizer(m1, [MiniBatch(x, y)], ClassNLLCriterion(), make(), batch_size=8)
        opt.setConstantGradientClipping(-0.05, 0.05).setGradientClippingByl2Norm(0.1)
        opt.prepare()
        for _ in range(3):
            opt.train_step(MiniBatch(x, y))
        assert calls == [["ConstantClippingProcessor", "L2NormClippingProcessor"]] * 3
        assert all(m.grad_clip is None for m in opt.optim_methods.values())
        # the update as it was: no clip settings, the processors run by hand where _clip runs
        ref = LocalOptimizer(m2, [MiniBatch(x, y)], ClassNLLCriterion(), make(), batch_size=8)
        ref._clip = lambda grad, shard: real([ConstantClippingProcessor(-0.05, 0.05), L2NormClippingProcessor(0.1)],
                                             None, grad)
        ref.prepare()
        for _ in range(3):
            ref.train_step(MiniBatch(x, y))
    got, want = _weights(m1), _weights(m2)
    assert not torch.equal(got, w0)
    assert torch.equal(got, want)


def _parse(argv):
    from bigdl.models.train.common import base_parser
    return base_parser("test", batch=8, epochs=1, lr=0.1).parse_args(argv)


class _Opt:
    constant_clip = None
    l2_clip = None

    def setConstantGradientClipping(self, lo, hi):
        self.constant_clip = (lo, hi)

    def setGradientClippingByl2Norm(self, thr):
        self.l2_clip = thr


@pytest.mark.parametrize("argv,const,l2", [
    ([], None, None),
    (["--gradientL2NormThreshold", "2.5"], None, 2.5),
    (["--gradientMin", "-1", "--gradientMax", "0.5"], (-1.0, 0.5), None),
    (["--gradientMin", "-1"], None, None),
    (["--gradientMax", "0.5"], None, None),
    (["--gradientMin", "-1", "--gradientMax", "0.5", "--gradientL2NormThreshold", "40"], (-1.0, 0.5), 40.0),
])
def test_cli_options_set_the_clipping(argv, const, l2):
    from bigdl.models.train.common import set_gradient_clipping
    opt = _Opt()
    set_gradient_clipping(opt, _parse(argv))
    assert opt.constant_clip == const and opt.l2_clip == l2


def test_cli_assemble_wires_a_real_optimizer():
    from bigdl.models.train.common import assemble
    from bigdl.nn import ClassNLLCriterion
    from bigdl import optim as O
    from bigdl.dataset import MiniBatch
    args = _parse(["--gradientMin", "-1", "--gradientMax", "1", "--gradientL2NormThreshold", "3"])
    with _cpu_engine():
        opt = assemble(_mlp(), [MiniBatch(torch.zeros(8, 16), torch.ones(8))], ClassNLLCriterion(),
                       O.SGD(learningrate=0.1), args)
    assert opt.constant_clip == (-1.0, 1.0) and opt.l2_clip == 3.0
    assert [type(p).__name__ for p in opt.parameter_processors()] == ["ConstantClippingProcessor",
                                                                      "L2NormClippingProcessor"]
