"""The one-pass update kernels of Adam, Adagrad, RMSprop, Adadelta, Adamax and Ftrl (the rules of
k_optim in csrc/optim_rules.hip) against the torch forms they replace on the GPU.

Kernel numerics are judged three ways from the same fp32 inputs: an fp64 oracle of the formula, the
fp32 torch form, and the kernel.  With E_t = max|torch_fp32 - oracle| per tensor, the kernel must
stay within 4·E_t + 1e-6 of the oracle: it evaluates the same formula in another rounding order
(fma contraction, sqrtf / powf / division within a few ulp), so its error is the size of the torch
form's and the factor 4 covers the four compounding steps; a wrong formula is off by 1e-3 or more.
A fixed tolerance would be wrong for Ftrl's ``linear``, where acc'^p - acc^p cancels.

Then: the bf16 gradient instances are bit-identical to the widened gradient, the device-counter
forms of Adam and Adagrad follow their host-scalar forms, the slice protocol leaves every element
outside the range untouched, unsupported operands are refused untouched by every wrapper, and the
methods agree with their torch form end to end (LocalOptimizer, and the DistriOptimizer's
sharded bf16 wire at world 1)."""
import contextlib
import copy
import functools
import math
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

STEPS = 4
SCALE = 0.5

# name -> hyper-parameters of the case
CASES = {
    "rmsprop": dict(kind="rmsprop", lr=0.01, decay=0.001, dr=0.99, eps=1e-8),
    "adadelta": dict(kind="adadelta", dr=0.9, eps=1e-6),
    "adamax": dict(kind="adamax", lr=0.002, b1=0.9, b2=0.999, eps=1e-38),
    "ftrl_p0.5": dict(kind="ftrl", lr=0.05, init=0.1, l1=1e-2, l2=1e-3, l2s=1e-4, power=-0.5),
    "ftrl_p0.3": dict(kind="ftrl", lr=0.05, init=0.1, l1=1e-2, l2=1e-3, l2s=1e-4, power=-0.3),
    "ftrl_p0": dict(kind="ftrl", lr=0.05, init=0.1, l1=1e-2, l2=1e-3, l2s=1e-4, power=0.0),
    "ftrl_nol2s": dict(kind="ftrl", lr=0.05, init=0.1, l1=1e-2, l2=1e-3, l2s=0.0, power=-0.5),
    "adam": dict(kind="adam", lr=1e-3, decay=0.001, b1=0.9, b2=0.999, eps=1e-8, wd=1e-3),
    "adagrad": dict(kind="adagrad", lr=0.01, decay=0.001, wd=1e-3),
}
STATES = {"rmsprop": ("sumSquare",), "adadelta": ("paramVariance", "delta"), "adamax": ("m", "u"),
          "ftrl": ("accum", "linear"), "adam": ("s", "r"), "adagrad": ("paramVariance",)}


def _native():
    from bigdl.ops import native, native_status
    st = native_status()
    assert st["loaded"], st
    return native


def _inputs(n):
    """(w0, [g_0 .. g_3]) on the host: every 7th element of every gradient exactly 0 (the elements
    never touched), the first 16 of step 0 too."""
    gen = torch.Generator().manual_seed(1234)
    w0 = torch.randn(n, generator=gen)
    grads = []
    for t in range(STEPS):
        g = torch.randn(n, generator=gen)
        g[::7] = 0
        if t == 0:
            g[:16] = 0
        grads.append(g)
    return w0, grads


def _init_states(hp, n, dtype, device="cpu"):
    st = [torch.zeros(n, dtype=dtype, device=device) for _ in STATES[hp["kind"]]]
    if hp["kind"] == "ftrl":
        st[0].fill_(hp["init"])
    return st


def _torch_form(hp, w, g, st, t):
    """Step ``t`` (0-based) of the method's torch form (optim/optim_method.py ``_update``), in the
    dtype of the operands: fp32 = the form the kernel replaces, fp64 = the oracle."""
    g = g.to(w.dtype) * SCALE
    k = hp["kind"]
    if k == "rmsprop":
        (s,) = st
        clr = hp["lr"] / (1 + t * hp["decay"])
        s.mul_(hp["dr"]).addcmul_(g, g, value=1 - hp["dr"])
        w.addcdiv_(g, s.sqrt().add_(hp["eps"]), value=-clr)
    elif k == "adadelta":
        v, d = st
        v.mul_(hp["dr"]).addcmul_(g, g, value=1 - hp["dr"])
        upd = (d + hp["eps"]).sqrt() / (v + hp["eps"]).sqrt() * g
        d.mul_(hp["dr"]).addcmul_(upd, upd, value=1 - hp["dr"])
        w.sub_(upd)
    elif k == "adamax":
        m, u = st
        m.mul_(hp["b1"]).add_(g, alpha=1 - hp["b1"])
        torch.maximum(u * hp["b2"], g.abs() + hp["eps"], out=u)
        w.addcdiv_(m, u, value=-hp["lr"] / (1 - hp["b1"] ** (t + 1)))
    elif k == "adam":  # ops/reference.py adam_step
        m, v = st
        g = g + hp["wd"] * w
        m.mul_(hp["b1"]).add_(g, alpha=1 - hp["b1"])
        v.mul_(hp["b2"]).addcmul_(g, g, value=1 - hp["b2"])
        clr = hp["lr"] / (1 + t * hp["decay"])
        step_size = clr * math.sqrt(1 - hp["b2"] ** (t + 1)) / (1 - hp["b1"] ** (t + 1))
        w.addcdiv_(m, v.sqrt().add_(hp["eps"]), value=-step_size)
    elif k == "adagrad":
        (s,) = st
        g = g + hp["wd"] * w
        s.addcmul_(g, g)
        w.addcdiv_(g, s.sqrt().add_(1e-10), value=-hp["lr"] / (1 + t * hp["decay"]))
    else:
        acc, lin = st
        gs = g + 2 * hp["l2s"] * w if hp["l2s"] > 0 else g
        new_acc = acc + g * g
        p = -hp["power"]
        sigma = (new_acc.pow(p) - acc.pow(p)) / hp["lr"]
        lin.add_(gs - sigma * w)
        quad = new_acc.pow(p) / hp["lr"] + 2 * hp["l2"]
        l1r = torch.clamp(lin.abs() - hp["l1"], min=0) * torch.sign(lin)
        w.copy_(torch.where(lin.abs() > hp["l1"], -l1r / quad, torch.zeros_like(w)))
        acc.copy_(new_acc)


def _kernel_step(hp, w, g, st, t, shadow):
    N = _native().native_ops
    k = hp["kind"]
    if k == "rmsprop":
        return N.rmsprop_step(w, g, st[0], hp["lr"] / (1 + t * hp["decay"]), hp["dr"], hp["eps"], SCALE, shadow)
    if k == "adadelta":
        return N.adadelta_step(w, g, st[0], st[1], hp["dr"], hp["eps"], SCALE, shadow)
    if k == "adamax":
        return N.adamax_step(w, g, st[0], st[1], hp["lr"], hp["b1"], hp["b2"], hp["eps"], t + 1, SCALE, shadow)
    if k == "adam":
        return N.adam_step(w, g, st[0], st[1], hp["lr"] / (1 + t * hp["decay"]), hp["b1"], hp["b2"], hp["eps"], t + 1,
                           hp["wd"], SCALE, shadow)
    if k == "adagrad":
        return N.adagrad_step(w, g, st[0], hp["lr"], hp["decay"], t, hp["wd"], SCALE, shadow)
    return N.ftrl_step(w, g, st[0], st[1], hp["lr"], hp["power"], hp["l1"], hp["l2"], hp["l2s"], SCALE, shadow)


def _grads16(grads, g16):
    """The gradients the kernel and both references see: rounded to bf16 first when ``g16``."""
    return [g.bfloat16() for g in grads] if g16 else grads


@functools.lru_cache(maxsize=None)
def _references(case, n, g16=False):
    """(oracle, torch_fp32): each ``[w, state...]`` after STEPS steps on the host, computed once per
    case and size and never modified."""
    hp = CASES[case]
    w0, grads = _inputs(n)
    grads = _grads16(grads, g16)
    out = []
    for dtype in (torch.float64, torch.float32):
        w, st = w0.to(dtype), _init_states(hp, n, dtype)
        for t, g in enumerate(grads):
            _torch_form(hp, w, g, st, t)
        out.append([w] + st)
    return out


@pytest.mark.parametrize("n", [1003, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_within_four_times_the_torch_forms_error(case, n):
    _check_against_oracle(case, n)


# the smallest length at which the grid-stride loop of k_optim (2048 blocks of 256 lanes, four
# elements each) runs a second pass, with a scalar tail: one full pass, 257 more float4s, one element
N_TWO_PASSES = 2048 * 256 * 4 + 1029


def test_grid_stride_second_pass_bf16_gradient():
    """The i += stride pass: Adam (two states), the bf16 gradient and the shadow, same bound."""
    _check_against_oracle("adam", N_TWO_PASSES, g16=True)


def _check_against_oracle(case, n, g16=False):
    hp = CASES[case]
    # the long case is used once: not kept in the cache
    oracle, t32 = (_references.__wrapped__ if n > 10000 else _references)(case, n, g16)
    w0, grads = _inputs(n)
    grads = _grads16(grads, g16)
    w = w0.to(dev)
    st = _init_states(hp, n, torch.float32, dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    for t, g in enumerate(grads):
        assert _kernel_step(hp, w, g.to(dev), st, t, shadow) is not NotImplemented
    torch.cuda.synchronize()
    got = [w.cpu()] + [s.cpu() for s in st]
    names = ("w",) + STATES[hp["kind"]]
    fails = []
    for name, k, o, r in zip(names, got, oracle, t32):
        assert torch.isfinite(k).all(), name
        e_t = float((r.double() - o).abs().max())
        e_k = float((k.double() - o).abs().max())
        bound = 4 * e_t + 1e-6
        print(f"optim_fused_error {case:<11} n={n:<5} {name:<13} torch_fp32={e_t:.3e} kernel={e_k:.3e} "
              f"kernel/bound={e_k / bound:.3f}")
        if not e_k <= bound:
            fails.append((name, e_k, bound))
    assert not fails, fails
    assert torch.equal(shadow.cpu(), got[0].bfloat16())
    if hp["kind"] == "adamax":
        # gradient exactly 0 at every step: m = 0, u = eps (a subnormal), w keeps its bits
        assert torch.equal(got[0][::7], w0[::7])
        assert torch.equal(got[2][::7], torch.full_like(got[2][::7], 1e-38))
    if hp["kind"] == "ftrl" and n > 100:
        zeros = int((got[0] == 0).sum())
        assert 0 < zeros < n, zeros  # both sides of the l1 test ran


BF16_CASES = ["rmsprop", "adadelta", "adamax", "ftrl_p0.5", "ftrl_p0.3", "adam", "adagrad"]


@pytest.mark.parametrize("case", BF16_CASES)
def test_bf16_gradient_is_the_widened_gradient_bit_for_bit(case):
    hp = CASES[case]
    n = 1003
    w0, grads = _inputs(n)
    g16 = grads[1].bfloat16().to(dev)
    outs = []
    for g in (g16, g16.float()):
        w = w0.to(dev)
        st = _init_states(hp, n, torch.float32, dev)
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        assert _kernel_step(hp, w, g, st, 0, shadow) is not NotImplemented
        outs.append([w, shadow] + st)
    torch.cuda.synchronize()
    assert not torch.equal(outs[0][0].cpu(), w0)
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


SLICE_CASES = ["rmsprop", "adadelta", "adamax", "ftrl_p0.5", "adam", "adagrad"]


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", SLICE_CASES)
def test_slice_update_leaves_the_rest_untouched(case, g_dtype):
    hp = CASES[case]
    total, lo, n = 2048, 16, 1003
    gen = torch.Generator().manual_seed(7)
    bufs = [torch.randn(total, generator=gen).to(dev)]                           # w
    bufs += [torch.rand(total, generator=gen).add_(0.1).to(dev) for _ in STATES[hp["kind"]]]
    shadow = torch.randn(total, generator=gen).bfloat16().to(dev)
    g = torch.randn(total, generator=gen).to(g_dtype).to(dev)
    before = [b.clone() for b in bufs] + [shadow.clone()]
    views = [b[lo:lo + n] for b in bufs]
    assert _kernel_step(hp, views[0], g[lo:lo + n], views[1:], 0, shadow[lo:lo + n]) is not NotImplemented
    torch.cuda.synchronize()
    for b, b0 in zip(bufs + [shadow], before):
        assert torch.equal(b[:lo], b0[:lo]) and torch.equal(b[lo + n:], b0[lo + n:])
        assert not torch.equal(b[lo:lo + n], b0[lo:lo + n])
    assert torch.equal(shadow[lo:lo + n], views[0].bfloat16())


@pytest.mark.parametrize("case", SLICE_CASES)
def test_unsupported_operands_are_refused_untouched(case):
    hp = CASES[case]
    n = 1003
    ns = len(STATES[hp["kind"]])
    w0 = torch.randn(n + 1, device=dev)
    g = torch.randn(n, device=dev)

    def states():
        return [torch.full((n,), 0.1, device=dev) for _ in range(ns)]

    # a weight view offset by one element: not 16-B aligned
    buf = w0.clone()
    assert _kernel_step(hp, buf[1:], g, states(), 0, None) is NotImplemented
    assert torch.equal(buf, w0)
    # a non-contiguous state
    w = w0[:n].clone()
    st = states()
    st[-1] = torch.full((2 * n,), 0.1, device=dev)[::2]
    assert _kernel_step(hp, w, g, st, 0, None) is NotImplemented
    assert torch.equal(w, w0[:n])
    # an fp16 gradient
    assert _kernel_step(hp, w, g.half(), states(), 0, None) is NotImplemented
    assert torch.equal(w, w0[:n])


@pytest.mark.parametrize("n", [1003, 3])
@pytest.mark.parametrize("case", ["adam", "adagrad"])
def test_device_counter_form_follows_the_host_scalar_form(case, n):
    """The iteration count read on the device (``prepare()`` of the rule forms the step size in
    fp32) against the same kernel with the step size formed on the host in double."""
    N = _native().native_ops
    hp = CASES[case]
    w0, grads = _inputs(n)
    runs = []
    for on_device in (False, True):
        w, st = w0.to(dev), _init_states(hp, n, torch.float32, dev)
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        nt = torch.zeros(1, device=dev)
        for t, g in enumerate(grads):
            g = g.to(dev)
            if not on_device:
                r = _kernel_step(hp, w, g, st, t, shadow)
            elif case == "adam":
                r = N.adam_step_dev(w, g, st[0], st[1], nt, hp["lr"], hp["decay"], hp["b1"], hp["b2"], hp["eps"],
                                    hp["wd"], SCALE, shadow)
            else:  # the host count (here a wrong one) is ignored when dev_n is given
                r = N.adagrad_step(w, g, st[0], hp["lr"], hp["decay"], 1000, hp["wd"], SCALE, shadow, dev_n=nt)
            assert r is not NotImplemented
            nt.add_(1)
        torch.cuda.synchronize()
        assert torch.equal(shadow, w.bfloat16())
        runs.append([w] + st)
    assert not torch.equal(runs[0][0].cpu(), w0)
    for host, devc in zip(*runs):
        torch.testing.assert_close(devc, host, rtol=1e-5, atol=1e-6)


def _wrapper_calls():
    """name -> (operand names, call(operands)) of the wrappers that share the operand contract with
    the rule kernels but are not reached through ``_kernel_step``'s cases."""
    N = _native().native_ops
    nt = torch.zeros(1, device=dev)
    return {
        "sgd_step": (("w", "g", "buf", "shadow"),
                     lambda o: N.sgd_step(o["w"], o["g"], o["buf"], 0.1, 0.9, 0.0, 1e-4, True, False, SCALE,
                                          o["shadow"])),
        "adam_step": (("w", "g", "m", "v", "shadow"),
                      lambda o: N.adam_step(o["w"], o["g"], o["m"], o["v"], 1e-3, 0.9, 0.999, 1e-8, 1, 1e-3, SCALE,
                                            o["shadow"])),
        "adam_step_dev": (("w", "g", "m", "v", "shadow"),
                          lambda o: N.adam_step_dev(o["w"], o["g"], o["m"], o["v"], nt, 1e-3, 0.0, 0.9, 0.999, 1e-8,
                                                    1e-3, SCALE, o["shadow"])),
        "adagrad_step": (("w", "g", "s", "shadow"),
                         lambda o: N.adagrad_step(o["w"], o["g"], o["s"], 0.01, 0.0, 0, 1e-3, SCALE, o["shadow"])),
    }


@pytest.mark.parametrize("wrapper", ["sgd_step", "adam_step", "adam_step_dev", "adagrad_step"])
def test_host_shadow_and_fp64_state_are_refused_untouched(wrapper):
    """One contract for every wrapper: a shadow in host memory and a state that is not fp32 never
    reach a kernel (it would read them as device bf16 / fp32), and no operand is written."""
    n = 1003
    names, call = _wrapper_calls()[wrapper]
    gen = torch.Generator().manual_seed(11)

    def operands():
        o = {k: torch.rand(n, generator=gen).add_(0.1).to(dev) for k in names}
        o["shadow"] = o["shadow"].bfloat16()
        return o

    state = names[2]
    for bad, make in (("shadow", lambda t: t.cpu()), (state, lambda t: t.double())):
        o = operands()
        o[bad] = make(o[bad])
        before = {k: v.clone() for k, v in o.items()}
        assert call(o) is NotImplemented, (wrapper, bad)
        torch.cuda.synchronize()
        for k in names:
            assert torch.equal(o[k], before[k]), (wrapper, bad, k)
    assert call(operands()) is not NotImplemented  # the same operands, well-formed, are taken


# ------------------------------------------------------------------------------------------- end to end
def _method(name):
    from bigdl import optim as O
    return {"rmsprop": lambda: O.RMSprop(learningrate=0.01, learningrate_decay=0.001),
            "adadelta": lambda: O.Adadelta(decayrate=0.9, epsilon=1e-6),
            "adamax": lambda: O.Adamax(learningrate=0.01),
            "ftrl": lambda: O.Ftrl(learningrate=0.05, l1_regularization_strength=1e-4,
                                   l2_regularization_strength=1e-3, l2_shrinkage_regularization_strength=1e-4),
            "adam": lambda: O.Adam(learningrate=0.01)}[name]()


class _Spy:
    """Counts the calls of a native wrapper (``ops.native_ops.<op>``) and what they returned."""

    def __init__(self, monkeypatch, op):
        from bigdl.ops import native_ops
        self.calls = []
        real = getattr(native_ops, op)

        def spy(w, g, *a, **k):
            r = real(w, g, *a, **k)
            self.calls.append((g.dtype, r is not NotImplemented))
            return r
        monkeypatch.setattr(native_ops, op, spy)

    @property
    def native(self):
        return [c for c in self.calls if c[1]]


def _convnet():
    from bigdl.nn import (Sequential, SpatialConvolution, ReLU, SpatialAveragePooling, View, Linear, LogSoftMax)
    from bigdl.utils.random import RNG
    RNG.setSeed(21)
    torch.manual_seed(21)
    return (Sequential().add(SpatialConvolution(3, 8, 3, 3)).add(ReLU()).add(SpatialAveragePooling(6, 6, 6, 6))
            .add(View(8)).add(Linear(8, 4)).add(LogSoftMax()))


def _weights(model):
    return torch.cat([p.detach().reshape(-1).float().cpu() for p in model.parameters()[0]])


@contextlib.contextmanager
def _compute(dtype):
    """Run with the compute dtype ``dtype`` on cuda:0, then put back what was set before."""
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    old_cfg, old_dt = config.get_property("bigdl.compute.dtype"), Engine.compute_dtype()
    config.set_property("bigdl.compute.dtype", dtype)
    Engine.set_compute_dtype(dtype)
    try:
        yield
    finally:
        config.set_property("bigdl.compute.dtype", old_cfg)
        Engine.set_compute_dtype(old_dt)


def _train_convnet(name, fused, dtype):
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    config.set_property("bigdl.optim.fused", fused)
    model = _convnet()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 8, 8, generator=gen).to(dev).to(Engine.compute_dtype())
    if dtype == "bf16":
        x = x.contiguous(memory_format=torch.channels_last)
    y = (torch.randint(0, 4, (8,), generator=gen) + 1).float().to(dev)
    opt = LocalOptimizer(model, [MiniBatch(x, y)], ClassNLLCriterion(), _method(name), batch_size=8)
    opt.prepare()
    assert opt.compute_dtype == (torch.float32 if dtype == "fp32" else torch.bfloat16)
    losses = [float(opt.train_step(MiniBatch(x, y))) for _ in range(3)]
    torch.cuda.synchronize()
    return losses, _weights(model)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["rmsprop", "adadelta", "adamax", "ftrl"])
def test_method_fused_matches_torch_form_under_local_optimizer(name, dtype, monkeypatch):
    from bigdl.utils import config
    _native()
    spy = _Spy(monkeypatch, name + "_step")
    with _compute(dtype):
        config.set_property("bigdl.deterministic", True)
        try:
            l_on, w_on = _train_convnet(name, True, dtype)
            assert len(spy.native) == 3 and len(spy.calls) == 3, spy.calls  # one native call per step
            l_off, w_off = _train_convnet(name, False, dtype)
            assert len(spy.calls) == 3, spy.calls                           # none with the property off
        finally:
            config.clear_property("bigdl.optim.fused")
            config.clear_property("bigdl.deterministic")
    print(f"{name} {dtype}: losses on={l_on} off={l_off} max|dw|={float((w_on - w_off).abs().max()):.3e}")
    assert all(l == l for l in l_on + l_off)
    assert l_on[0] != l_on[2] and l_off[0] != l_off[2]  # the forward saw the updated weights
    torch.testing.assert_close(w_on, w_off, rtol=2e-4, atol=2e-5)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _mlp():
    from bigdl.nn import Sequential, Linear, Tanh, LogSoftMax
    from bigdl.utils.random import RNG
    RNG.setSeed(7)
    torch.manual_seed(7)
    return Sequential().add(Linear(8, 16)).add(Tanh()).add(Linear(16, 4)).add(LogSoftMax())


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_sharded_bf16_wire_reads_the_wire_shard_at_world_1(name, monkeypatch):
    """DistriOptimizer, sharded, bf16 gradient wire, world 1 without aliasing: the update kernel
    reads the bf16 reduce-scatter shard itself (no fp32 unpack) and the run follows the
    LocalOptimizer's within the wire's rounding."""
    _native()
    with _compute("bf16"):
        _sharded_world1(name, monkeypatch)


def _sharded_world1(name, monkeypatch):
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    m1 = _mlp()
    m2 = copy.deepcopy(m1)
    w0 = _weights(m1)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(8, 8, generator=gen).to(dev).to(Engine.compute_dtype())
    y = (torch.randint(0, 4, (8,), generator=gen) + 1).float().to(dev)
    local = LocalOptimizer(m1, [MiniBatch(x, y)], ClassNLLCriterion(), _method(name), batch_size=8)
    local.prepare()
    for _ in range(3):
        local.train_step(MiniBatch(x, y))
    torch.cuda.synchronize()
    ref = _weights(m1)

    spy = _Spy(monkeypatch, name + "_step")
    if name == "adam":
        # Adam goes through the dispatcher (ops.adam_step), which binds the wrapper at import:
        # route it through the spied wrapper, then on to the dispatcher if that refuses
        import bigdl.ops as ops
        from bigdl.ops import native_ops
        real_dispatch = ops.adam_step

        def dispatch(*a, **k):
            r = native_ops.adam_step(*a, **k)
            return r if r is not NotImplemented else real_dispatch(*a, **k)
        monkeypatch.setattr(ops, "adam_step", dispatch)
    saved = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    config.set_property("bigdl.comm.aliasWorld1", False)
    config.set_property("bigdl.comm.dtype", "bf16")
    config.set_property("bigdl.comm.sharded", True)
    try:
        Engine.init(device="cuda:0", dist=True)
        from bigdl.parallel import DistriOptimizer
        distri = DistriOptimizer(m2, [MiniBatch(x, y)], ClassNLLCriterion(), _method(name), batch_size=8)
        distri.prepare()
        assert distri.sharded and not distri._alias and distri.grad_wire is not None
        for _ in range(3):
            distri.train_step(MiniBatch(x, y))
        distri._finish()
        torch.cuda.synchronize()
    finally:
        Engine.shutdown()
        for k in ("bigdl.comm.aliasWorld1", "bigdl.comm.dtype", "bigdl.comm.sharded"):
            config.clear_property(k)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        Engine.init(device="cuda:0")
    got = _weights(m2)
    refused = [c for c in spy.calls if not c[1]]
    print(f"{name}: {len(spy.calls)} shard calls, {len(refused)} fell back (alignment), "
          f"{sum(1 for c in spy.native if c[0] == torch.bfloat16)} native with a bf16 gradient")
    assert any(c[0] == torch.bfloat16 for c in spy.native), spy.calls
    assert not torch.equal(ref, w0)
    cos = float(torch.nn.functional.cosine_similarity(got - w0, ref - w0, dim=0))
    assert cos > 0.99, cos
