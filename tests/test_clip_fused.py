"""Fused gradient clipping on the GPU: the deterministic Σg² kernel (csrc/clip.hip), the GradClip
operand of every update kernel (k_sgd, every rule of k_optim), and the one decision point of the
Local and Distri optimizers.

The oracle is what ``run_processors([ConstantClipping, L2NormClipping])`` does to g·grad_scale, in
fp64: clamp(g·scale, lo, hi)·min(1, thr / (‖g‖·scale + 1e-6)), the norm taken before the clamp.
Bit-exact claims (a clamp alone, an L2 threshold that does not bite) are checked against the
UNCLIPPED kernels, so they hold the clipped instances to the parent's arithmetic; the active L2
scale is judged like tests/test_optim_fused.py judges the rules: within 4·E_torch + 1e-6 of fp64."""
import contextlib
import importlib.util
import math
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

# the rule cases, inputs and torch forms of tests/test_optim_fused.py, in a private copy of that
# module whose gradient scale is 1: here the gradient reaches the torch form already scaled and clipped
_spec = importlib.util.spec_from_file_location(
    "_optim_fused_forms", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_optim_fused.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
T.SCALE = 1.0

STEPS = T.STEPS
SCALE = 0.5
LO, HI = -0.3, 0.2
N = 4099  # 1024 float4s (more than one block) + a 3-element tail
U = 2.0 ** -24

_SGD = dict(kind="sgd", lr=0.05, mom=0.0, damp=0.0, wd=1e-3, nesterov=False, perelem=False)
CASES = dict(T.CASES)
CASES.update({
    "sgd_plain": dict(_SGD),
    "sgd_momentum": dict(_SGD, mom=0.9, damp=0.1),
    "sgd_nesterov": dict(_SGD, mom=0.9, nesterov=True),
    "sgd_perelem": dict(_SGD, mom=0.9, wd=1.0, perelem=True),
})
STATES = dict(T.STATES, sgd=("dfdx",))


def _native():
    return T._native()


def _ops():
    return _native().native_ops


def _clip_cls():
    from bigdl.parameters import GradClip
    return GradClip


# ------------------------------------------------------------------------------------------- Σg²
def _depth(n):
    """Addition depth D of ``grad_sumsq`` for n elements, as csrc/clip.hip states it:
    D = I + 1 + 2 + 6 + 2 + ceil(G/64) + 6 with G = min(2048, ceil((n/4)/256)) blocks and
    I = ceil((n/4) / (256·G)) terms per accumulator."""
    n4 = n // 4
    g = min(2048, max(1, -(-n4 // 256)))
    i = max(1, -(-n4 // (256 * g)))
    return i + 1 + 2 + 6 + 2 + -(-g // 64) + 6


SUMSQ_SIZES = [1, 3, 4, 5, 255, 1027, 3 * 8192 + 5, 2 ** 20 + 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_grad_sumsq_against_fp64(n, dtype):
    ops = _ops()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dtype)
    want = float(g.double().square().sum())  # bf16: the widened values, squared in fp64
    gd = g.to(dev)
    out = torch.full((1,), -1.0, device=dev)
    partials = torch.empty(ops.SUMSQ_PARTIALS, device=dev)
    assert ops.grad_sumsq(gd, out, partials) is out
    a = out.clone()
    out.fill_(-1.0)
    partials.fill_(float("nan"))  # scratch: what it held before must not matter
    assert ops.grad_sumsq(gd, out, partials) is out
    torch.cuda.synchronize()
    got = float(out)
    d = _depth(n)
    rel = abs(got - want) / want
    print(f"clip_fused_error grad_sumsq n={n:<8} {str(dtype).replace('torch.', ''):<8} D={d:<3} rel={rel:.3e} "
          f"rel/bound={rel / (d * U):.3f}")
    assert rel <= d * U
    assert torch.equal(a, out)  # the same bits from run to run
    fresh = ops.grad_sumsq(gd)  # buffers made by the wrapper
    assert torch.equal(fresh, out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_grad_sumsq_of_a_slice_inside_an_arena(dtype):
    ops = _ops()
    lo, n = 8, 1027
    arena = torch.full((lo + n + 64,), 1000.0)  # guards on both sides: one of them would add 1e6
    body = torch.randn(n, generator=torch.Generator().manual_seed(9))
    arena[lo:lo + n] = body
    arena = arena.to(dtype).to(dev)
    want = float(arena[lo:lo + n].double().square().sum())
    out = ops.grad_sumsq(arena[lo:lo + n])
    assert out is not NotImplemented
    rel = abs(float(out) - want) / want
    assert rel <= _depth(n) * U, rel
    # a start that is not 16-B (fp32) / 8-B (bf16) aligned is refused, as is a strided view
    assert ops.grad_sumsq(arena[lo + 1:lo + 1 + n]) is NotImplemented
    assert ops.grad_sumsq(arena[::2]) is NotImplemented
    assert ops.grad_sumsq(arena[lo:lo + n], torch.zeros(2, device=dev)) is NotImplemented


# ------------------------------------------------------------------------------------------- kernels
def _perelem(n):
    gen = torch.Generator().manual_seed(77)
    return torch.rand(n, generator=gen) + 0.5, torch.rand(n, generator=gen) * 1e-3


def _init_states(hp, n, dtype, device="cpu"):
    if hp["kind"] == "sgd":
        return [torch.zeros(n, dtype=dtype, device=device)]
    return T._init_states(hp, n, dtype, device)


def _kernel_step(hp, w, g, st, t, shadow, scale, clip):
    """One update by the native wrapper with gradient scale ``scale`` and the clip operand."""
    ops = _ops()
    k = hp["kind"]
    if k == "sgd":
        lrs = wds = None
        if hp["perelem"]:
            lrs, wds = (v.to(w.device) for v in _perelem(w.numel()))
        return ops.sgd_step(w, g, st[0] if hp["mom"] else None, hp["lr"], hp["mom"], hp["damp"], hp["wd"],
                            hp["nesterov"], t == 0, scale, shadow, lrs, wds, clip=clip)
    if k == "rmsprop":
        return ops.rmsprop_step(w, g, st[0], hp["lr"] / (1 + t * hp["decay"]), hp["dr"], hp["eps"], scale, shadow,
                                clip=clip)
    if k == "adadelta":
        return ops.adadelta_step(w, g, st[0], st[1], hp["dr"], hp["eps"], scale, shadow, clip=clip)
    if k == "adamax":
        return ops.adamax_step(w, g, st[0], st[1], hp["lr"], hp["b1"], hp["b2"], hp["eps"], t + 1, scale, shadow,
                               clip=clip)
    if k == "adam":
        return ops.adam_step(w, g, st[0], st[1], hp["lr"] / (1 + t * hp["decay"]), hp["b1"], hp["b2"], hp["eps"],
                             t + 1, hp["wd"], scale, shadow, clip=clip)
    if k == "adagrad":
        return ops.adagrad_step(w, g, st[0], hp["lr"], hp["decay"], t, hp["wd"], scale, shadow, clip=clip)
    return ops.ftrl_step(w, g, st[0], st[1], hp["lr"], hp["power"], hp["l1"], hp["l2"], hp["l2s"], scale, shadow,
                         clip=clip)


def _torch_form(hp, w, g, st, t):
    """Step ``t`` of the torch form over the already scaled and clipped gradient ``g``, in the
    dtype of the operands (fp32: the form the kernel replaces; fp64: the oracle).  The rules are
    those of tests/test_optim_fused.py; SGD is ops/reference.py sgd_step written for either dtype."""
    if hp["kind"] != "sgd":
        return T._torch_form(hp, w, g, st, t)
    g = g.to(w.dtype)
    lrs, wds = (v.to(w.dtype) for v in _perelem(w.numel())) if hp["perelem"] else (1.0, 1.0)
    gg = g + hp["wd"] * wds * w
    d = gg
    if hp["mom"]:
        buf = st[0]
        if t == 0:
            buf.copy_(gg)
        else:
            buf.mul_(hp["mom"]).add_(gg, alpha=1 - hp["damp"])
        d = gg + hp["mom"] * buf if hp["nesterov"] else buf
    w.sub_(hp["lr"] * lrs * d)


def _grads(n, g16):
    w0, grads = T._inputs(n)
    return w0, ([g.bfloat16() for g in grads] if g16 else grads)


def _run_kernel(hp, w0, grads, scale, clip_for):
    """STEPS updates on the device; ``clip_for(t, g_dev)`` gives the step's clip operand (or None).
    Returns [w, shadow, state...] on the host."""
    n = w0.numel()
    w = w0.to(dev)
    st = _init_states(hp, n, torch.float32, dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    for t, g in enumerate(grads):
        gd = g.to(dev)
        assert _kernel_step(hp, w, gd, st, t, shadow, scale, clip_for(t, gd)) is not NotImplemented
    torch.cuda.synchronize()
    assert torch.equal(shadow, w.bfloat16())
    return [w.cpu(), shadow.cpu()] + [s.cpu() for s in st]


def _assert_same_bits(got, want, w0):
    assert not torch.equal(got[0], w0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a.float()).all(), i
        assert torch.equal(a, b), (i, float((a.double() - b.double()).abs().max()))


@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g16"])
@pytest.mark.parametrize("case", list(CASES))
def test_clamp_only_is_the_unclipped_kernel_on_the_clamped_gradient(case, g16):
    """One rounding in g·scale, an exact clamp and an exact ·1: the clipped kernel must give the
    bits of the unclipped kernel fed (g.float()·scale).clamp(lo, hi) with scale 1 — weights, every
    state and the shadow."""
    hp = CASES[case]
    w0, grads = _grads(N, g16)
    clip = _clip_cls()(None, LO, HI)
    got = _run_kernel(hp, w0, grads, SCALE, lambda t, g: clip)
    clamped = [(g.float() * SCALE).clamp(LO, HI) for g in grads]
    assert all(not torch.equal(c, g.float() * SCALE) for c, g in zip(clamped, grads))  # the clamp bites
    want = _run_kernel(hp, w0, clamped, 1.0, lambda t, g: None)
    _assert_same_bits(got, want, w0)


@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g16"])
@pytest.mark.parametrize("case", list(CASES))
def test_inactive_l2_is_the_unclipped_kernel(case, g16):
    """threshold = 2·‖g·scale‖ (fp64): s = min(1, ≈2) is exactly 1 and the bounds are ±inf, so the
    clipped kernel must give the bits of the unclipped one (g·0.5 is exact, so rounding it before
    the rule's multiply-add changes nothing)."""
    hp = CASES[case]
    w0, grads = _grads(N, g16)
    ops = _ops()
    sumsq = torch.zeros(1, device=dev)
    partials = torch.empty(ops.SUMSQ_PARTIALS, device=dev)

    def clip_for(t, gd):
        assert ops.grad_sumsq(gd, sumsq, partials) is sumsq
        thr = 2.0 * float(grads[t].double().square().sum().sqrt()) * SCALE
        return _clip_cls()(thr, sumsq=sumsq, partials=partials)
    got = _run_kernel(hp, w0, grads, SCALE, clip_for)
    want = _run_kernel(hp, w0, grads, SCALE, lambda t, g: None)
    _assert_same_bits(got, want, w0)


@pytest.mark.parametrize("g16", [False, True], ids=["g32", "g16"])
@pytest.mark.parametrize("clamp", [False, True], ids=["l2", "l2+clamp"])
@pytest.mark.parametrize("case", list(CASES))
def test_active_l2_within_four_times_the_torch_forms_error(case, clamp, g16):
    """threshold = 0.5·‖g·scale‖: the L2 scale is about 0.5 in every arm (no branch can flip).
    The oracle (fp64) and the fp32 torch form (GradClip.apply, then the method's torch form) take
    Σg² from the device buffer the kernel read, which isolates the update's arithmetic from the
    reduction's (judged by test_grad_sumsq_against_fp64).  Per tensor: 4·E_torch + 1e-6."""
    hp = CASES[case]
    GradClip = _clip_cls()
    ops = _ops()
    lo, hi = (LO, HI) if clamp else (-math.inf, math.inf)
    w0, grads = _grads(N, g16)
    thrs = [0.5 * float(g.double().square().sum().sqrt()) * SCALE for g in grads]
    sumsq = torch.zeros(1, device=dev)
    partials = torch.empty(ops.SUMSQ_PARTIALS, device=dev)
    seen = []

    def clip_for(t, gd):
        assert ops.grad_sumsq(gd, sumsq, partials) is sumsq
        seen.append(sumsq.cpu().clone())
        return GradClip(thrs[t], lo, hi, sumsq=sumsq, partials=partials)
    got = _run_kernel(hp, w0, grads, SCALE, clip_for)
    got = [got[0]] + got[2:]

    # fp64 oracle and the fp32 torch form, both from the Σg² the kernel read
    w64, st64 = w0.double(), _init_states(hp, N, torch.float64)
    w32, st32 = w0.clone(), _init_states(hp, N, torch.float32)
    for t, g in enumerate(grads):
        norm = math.sqrt(float(seen[t])) * SCALE
        s = min(1.0, thrs[t] / (norm + 1e-6))
        assert 0.45 < s < 0.55, s
        _torch_form(hp, w64, (g.double() * SCALE).clamp(lo, hi) * s, st64, t)
        c32 = GradClip(thrs[t], lo, hi, sumsq=seen[t])
        _torch_form(hp, w32, c32.apply(g.float() * SCALE, SCALE), st32, t)
    names = ("w",) + STATES[hp["kind"]]
    fails = []
    for name, k, o, r in zip(names, got, [w64] + st64, [w32] + st32):
        assert torch.isfinite(k).all(), name
        e_t = float((r.double() - o).abs().max())
        e_k = float((k.double() - o).abs().max())
        bound = 4 * e_t + 1e-6
        print(f"clip_fused_error active_l2 {case:<12} {'l2+clamp' if clamp else 'l2':<8} {'g16' if g16 else 'g32'} "
              f"{name:<13} torch_fp32={e_t:.3e} kernel={e_k:.3e} kernel/bound={e_k / bound:.3f}")
        if not e_k <= bound:
            fails.append((name, e_k, bound))
    assert not fails, fails
    assert not torch.equal(got[0], w0)


def test_adam_device_counter_form_takes_the_clip():
    """bigdl_adam_dev's clipped form: clamp-only, against the unclipped device-counter kernel on
    the clamped gradient, bit for bit."""
    ops = _ops()
    hp = CASES["adam"]
    w0, grads = _grads(N, False)
    clip = _clip_cls()(None, LO, HI)
    outs = []
    for clipped in (True, False):
        w, st = w0.to(dev), _init_states(hp, N, torch.float32, dev)
        shadow = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        nt = torch.zeros(1, device=dev)
        for g in grads:
            g = g.to(dev)
            if not clipped:
                g = (g * SCALE).clamp(LO, HI)
            r = ops.adam_step_dev(w, g, st[0], st[1], nt, hp["lr"], hp["decay"], hp["b1"], hp["b2"], hp["eps"],
                                  hp["wd"], SCALE if clipped else 1.0, shadow, clip=clip if clipped else None)
            assert r is not NotImplemented
            nt.add_(1)
        torch.cuda.synchronize()
        outs.append([w.cpu(), shadow.cpu()] + [s.cpu() for s in st])
    _assert_same_bits(outs[0], outs[1], w0)


def _wrappers():
    """name -> (operand names, call(operands, clip)) of every ``*_step`` wrapper."""
    ops = _ops()
    nt = torch.zeros(1, device=dev)
    return {
        "sgd_step": (("w", "g", "a"), lambda o, c: ops.sgd_step(o["w"], o["g"], o["a"], 0.1, 0.9, 0.0, 1e-4, True,
                                                                False, SCALE, None, clip=c)),
        "adam_step": (("w", "g", "a", "b"), lambda o, c: ops.adam_step(o["w"], o["g"], o["a"], o["b"], 1e-3, 0.9,
                                                                       0.999, 1e-8, 1, 1e-3, SCALE, None, clip=c)),
        "adam_step_dev": (("w", "g", "a", "b"),
                          lambda o, c: ops.adam_step_dev(o["w"], o["g"], o["a"], o["b"], nt, 1e-3, 0.0, 0.9, 0.999,
                                                         1e-8, 1e-3, SCALE, None, clip=c)),
        "adagrad_step": (("w", "g", "a"), lambda o, c: ops.adagrad_step(o["w"], o["g"], o["a"], 0.01, 0.0, 0, 1e-3,
                                                                        SCALE, None, clip=c)),
        "rmsprop_step": (("w", "g", "a"), lambda o, c: ops.rmsprop_step(o["w"], o["g"], o["a"], 0.01, 0.99, 1e-8,
                                                                        SCALE, None, clip=c)),
        "adadelta_step": (("w", "g", "a", "b"), lambda o, c: ops.adadelta_step(o["w"], o["g"], o["a"], o["b"], 0.9,
                                                                               1e-6, SCALE, None, clip=c)),
        "adamax_step": (("w", "g", "a", "b"), lambda o, c: ops.adamax_step(o["w"], o["g"], o["a"], o["b"], 0.002, 0.9,
                                                                           0.999, 1e-38, 1, SCALE, None, clip=c)),
        "ftrl_step": (("w", "g", "a", "b"), lambda o, c: ops.ftrl_step(o["w"], o["g"], o["a"], o["b"], 0.05, -0.5,
                                                                       1e-2, 1e-3, 1e-4, SCALE, None, clip=c)),
    }


@pytest.mark.parametrize("wrapper", ["sgd_step", "adam_step", "adam_step_dev", "adagrad_step", "rmsprop_step",
                                     "adadelta_step", "adamax_step", "ftrl_step"])
def test_malformed_sumsq_is_refused_untouched(wrapper):
    """The clip operand is part of the one operand contract: a Σg² scalar in host memory, in fp64
    or of two elements never reaches a kernel, and no operand is written."""
    GradClip = _clip_cls()
    n = 1003
    names, call = _wrappers()[wrapper]
    gen = torch.Generator().manual_seed(11)

    def operands():
        return {k: torch.rand(n, generator=gen).add_(0.1).to(dev) for k in names}

    bad = {"host": torch.ones(1), "fp64": torch.ones(1, dtype=torch.float64, device=dev),
           "two": torch.ones(2, device=dev)}
    for why, sq in bad.items():
        o = operands()
        before = {k: v.clone() for k, v in o.items()}
        assert call(o, GradClip(1.0, sumsq=sq)) is NotImplemented, (wrapper, why)
        torch.cuda.synchronize()
        for k in names:
            assert torch.equal(o[k], before[k]), (wrapper, why, k)
    o = operands()
    w_before = o["w"].clone()
    assert call(o, GradClip(1.0, sumsq=torch.ones(1, device=dev))) is not NotImplemented  # well-formed: taken
    assert not torch.equal(o["w"], w_before)


# ------------------------------------------------------------------------------------------- end to end
CONST = (-0.05, 0.05)
L2 = 0.1
IN, HID, OUT, BATCH = 16, 32, 4, 8
N_MLP = IN * HID + HID + HID * OUT + OUT


def _mlp():
    from bigdl.nn import Sequential, Linear, Tanh, LogSoftMax
    from bigdl.utils.random import RNG
    RNG.setSeed(7)
    torch.manual_seed(7)
    return Sequential().add(Linear(IN, HID)).add(Tanh()).add(Linear(HID, OUT)).add(LogSoftMax())


def _params(model):
    return [p.detach().float().cpu().clone() for p in model.parameters()[0]]


def _flat(ps):
    return torch.cat([p.reshape(-1) for p in ps])


def _batch(dtype=torch.float32):
    """Inputs scaled by 10 so that the gradient norm is far above the threshold."""
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(BATCH, IN, generator=gen) * 10).to(dtype)
    y = (torch.randint(0, OUT, (BATCH,), generator=gen) + 1).float()
    return x, y


def _method(name):
    from bigdl import optim as O
    return {"sgd": lambda: O.SGD(learningrate=0.1, momentum=0.9, dampening=0.0),
            "adam": lambda: O.Adam(learningrate=0.01)}[name]()


def _oracle(name, params0, x, y, const, l2, steps=3):
    """The fp64 trajectory: the MLP's gradient by autograd, the two processors (norm before the
    clamp, + 1e-6), then momentum SGD (v = g at the first step) or Adam."""
    ps = [p.double().clone().requires_grad_(True) for p in params0]
    x = x.double()
    tgt = (y - 1).long()
    state = {}
    for t in range(steps):
        w1, b1, w2, b2 = ps
        logp = torch.log_softmax(torch.tanh(x @ w1.t() + b1) @ w2.t() + b2, dim=1)
        loss = -logp[torch.arange(BATCH), tgt].mean()
        gs = torch.autograd.grad(loss, ps)
        g = _flat([v.detach() for v in gs])
        norm = float(g.square().sum().sqrt())
        assert l2 is None or norm > 4 * l2, norm  # the threshold bites, and no arm's branch can flip
        if const is not None:
            g = g.clamp(*const)
        if l2 is not None:
            g = g * min(1.0, l2 / (norm + 1e-6))
        w = _flat([p.detach() for p in ps])
        if name == "sgd":
            v = g.clone() if t == 0 else 0.9 * state["v"] + g
            state["v"] = v
            w = w - 0.1 * v
        else:
            m = state.get("m", torch.zeros_like(w)) * 0.9 + 0.1 * g
            v = state.get("v", torch.zeros_like(w)) * 0.999 + 0.001 * g * g
            state["m"], state["v"] = m, v
            step = 0.01 * math.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1))
            w = w - step * m / (v.sqrt() + 1e-8)
        off = 0
        new = []
        for p in ps:
            new.append(w[off:off + p.numel()].reshape(p.shape).clone().requires_grad_(True))
            off += p.numel()
        ps = new
    return _flat([p.detach() for p in ps])


class _ProcSpy:
    def __init__(self, monkeypatch):
        import bigdl.parameters as P
        self.calls = 0
        real = P.run_processors

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(P, "run_processors", spy)


def _share(w_oracle, w0):
    """What the reduction's error may add to the fused arm's weight error.  The L2 scale is
    s = thr / (sqrtf(Σ)·scale + 1e-6).  Σ carries a relative error of at most D·2⁻²⁴ (the kernel's
    stated depth), the square root halves it, and sqrtf, the multiply, the add and the divide
    round once each at 2⁻²⁵ relative: 4·2⁻²⁵ = 2⁻²³.  An update is at most proportional to the
    clipped gradient (SGD: exactly, momentum included, since every step carries the same factor;
    Adam: less, its step is invariant to the gradient's scale), so a relative error ε in s moves
    the weights by at most ε·|Δw|: share = (D·2⁻²⁴/2 + 2⁻²³)·max|Δw|, Δw the oracle's movement."""
    return (_depth(N_MLP) * U / 2 + 2.0 ** -23) * float((w_oracle - w0.double()).abs().max())


def _check_arms(tag, w_fused, w_proc, w_oracle, w0):
    e_f = float((w_fused.double() - w_oracle).abs().max())
    e_p = float((w_proc.double() - w_oracle).abs().max())
    share = _share(w_oracle, w0)
    bound = 4 * e_p + 1e-6 + share
    print(f"clip_fused_error end_to_end {tag:<28} processors={e_p:.3e} fused={e_f:.3e} share={share:.3e} "
          f"fused/bound={e_f / bound:.3f}")
    assert float((w_oracle - w0.double()).abs().max()) > 1e-4  # the run moved the weights: 100 × the 1e-6 floor
    assert e_f <= bound, (e_f, bound)


def _train_local(name, fused, const, l2):
    from bigdl.utils import config
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    config.set_property("bigdl.clip.fused", fused)
    model = _mlp()
    p0 = _params(model)
    x, y = _batch()
    xb, yb = x.to(dev), y.to(dev)
    opt = LocalOptimizer(model, [MiniBatch(xb, yb)], ClassNLLCriterion(), _method(name), batch_size=BATCH)
    if const is not None:
        opt.setConstantGradientClipping(*const)
    if l2 is not None:
        opt.setGradientClippingByl2Norm(l2)
    opt.prepare()
    assert opt.compute_dtype == torch.float32
    for _ in range(3):
        opt.train_step(MiniBatch(xb, yb))
    torch.cuda.synchronize()
    assert [type(p).__name__ for p in opt.parameter_processors()] == \
        ["ConstantClippingProcessor"] * (const is not None) + ["L2NormClippingProcessor"] * (l2 is not None)
    return p0, _flat(_params(model)), opt


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_local_optimizer_fused_against_the_processors(name, monkeypatch):
    """Both clippings, 3 steps from the same init with ``bigdl.clip.fused`` on and off, each arm
    against the fp64 trajectory: the fused arm within 4× the processor arm's error + 1e-6 + the
    share of the reduction's error (``_share``).  With the property on, ``run_processors`` never
    runs; with it off, it runs every step."""
    from bigdl.utils import config
    _native()
    spy = _ProcSpy(monkeypatch)
    with T._compute("fp32"):
        try:
            p0, w_on, opt = _train_local(name, True, CONST, L2)
            assert spy.calls == 0
            assert all(m.grad_clip is not None for m in opt.optim_methods.values())
            _, w_off, opt = _train_local(name, False, CONST, L2)
            assert spy.calls == 3
            assert all(m.grad_clip is None for m in opt.optim_methods.values())
        finally:
            config.clear_property("bigdl.clip.fused")
    x, y = _batch()
    _check_arms(f"local {name}", w_on, w_off, _oracle(name, p0, x, y, CONST, L2), _flat(p0))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@contextlib.contextmanager
def _world1():
    """A one-rank process group, sharded, bf16 gradient wire, the shard NOT aliased to the arena
    (as test_optim_fused.py sets it up), bf16 compute; everything is put back afterwards."""
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    props = {"bigdl.comm.aliasWorld1": False, "bigdl.comm.dtype": "bf16", "bigdl.comm.sharded": True,
             "bigdl.comm.overlap": True, "bigdl.comm.earlyUpdate": True, "bigdl.deterministic": True}
    with T._compute("bf16"):
        saved = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(_free_port()))
        for k, v in props.items():
            config.set_property(k, v)
        try:
            Engine.init(device="cuda:0", dist=True)
            yield
        finally:
            Engine.shutdown()
            for k in list(props) + ["bigdl.clip.fused"]:
                config.clear_property(k)
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            Engine.init(device="cuda:0")


def _train_distri(method, fused, const, l2, steps=3):
    """(initial params, final weights, per-step observations) of a DistriOptimizer run."""
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.nn import ClassNLLCriterion
    from bigdl.parallel import DistriOptimizer
    from bigdl.dataset import MiniBatch
    config.set_property("bigdl.clip.fused", fused)
    model = _mlp()
    p0 = _params(model)
    x, y = _batch(torch.bfloat16)
    xb, yb = x.to(dev).to(Engine.compute_dtype()), y.to(dev)
    meth = method(model) if callable(method) else _method(method)
    distri = DistriOptimizer(model, [MiniBatch(xb, yb)], ClassNLLCriterion(), meth, batch_size=BATCH)
    if const is not None:
        distri.setConstantGradientClipping(*const)
    if l2 is not None:
        distri.setGradientClippingByl2Norm(l2)
    distri.prepare()
    assert distri.sharded and not distri._alias and distri.grad_wire is not None
    seen = []
    for _ in range(steps):
        distri.train_step(MiniBatch(xb, yb))
        seen.append(dict(unpacked=any(b.unpacked for b in distri.buckets), early=distri._early,
                         overlap=distri._overlap_active, early_buckets=sum(1 for b in distri.buckets if b.early)))
    distri._finish()
    torch.cuda.synchronize()
    return p0, _flat(_params(model)), seen, distri


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_sharded_bf16_wire_fused_against_the_processors(name, monkeypatch):
    """DistriOptimizer at world 1, sharded, bf16 wire: the same comparison and bound as the local
    test.  Fused, the sum of squares and every update read the bf16 wire shard: no bucket is
    unpacked and the processors never run."""
    _native()
    spy = _ProcSpy(monkeypatch)
    with _world1():
        p0, w_on, seen_on, opt = _train_distri(name, True, CONST, L2)
        assert spy.calls == 0
        assert not any(s["unpacked"] for s in seen_on), seen_on
        assert not any(s["early"] for s in seen_on), seen_on  # an L2 threshold keeps early updates off
        assert all(m.grad_clip is not None for m in opt.optim_methods.values())
        _, w_off, seen_off, _ = _train_distri(name, False, CONST, L2)
        assert spy.calls == 3
        assert all(s["unpacked"] for s in seen_off), seen_off  # the processor path does unpack
    x, y = _batch(torch.bfloat16)
    _check_arms(f"distri {name}", w_on, w_off, _oracle(name, p0, x.float(), y, CONST, L2), _flat(p0))


def test_sharded_constant_clamp_keeps_early_updates(monkeypatch):
    """A constant clamp needs nothing global: fused, the in-backward (early) shard updates stay on
    once overlap is active (after the first iteration), and the result follows the processors'."""
    _native()
    spy = _ProcSpy(monkeypatch)
    with _world1():
        p0, w_on, seen_on, _ = _train_distri("sgd", True, CONST, None)
        assert spy.calls == 0
        assert not seen_on[0]["overlap"] and not seen_on[0]["early"]
        for s in seen_on[1:]:
            assert s["overlap"] and s["early"] and s["early_buckets"] > 0 and not s["unpacked"], seen_on
        _, w_off, seen_off, _ = _train_distri("sgd", False, CONST, None)
        assert spy.calls == 3
        assert not any(s["early"] for s in seen_off), seen_off
    x, y = _batch(torch.bfloat16)
    _check_arms("distri sgd clamp-only early", w_on, w_off, _oracle("sgd", p0, x.float(), y, CONST, None), _flat(p0))


def test_sharded_lars_with_clipping_keeps_the_processor_path(monkeypatch):
    """LarsSGD is out of the fused path (its layer norms would have to be those of the clipped
    gradient): whatever ``bigdl.clip.fused`` says, the processors run over the unpacked fp32 shard
    as before, no method carries a clip operand, and the weights are the same bit for bit."""
    from bigdl.optim import LarsSGD
    _native()
    spy = _ProcSpy(monkeypatch)

    def lars(model):
        return LarsSGD.createOptimForModule(model, learningRate=0.05, learningRateDecay=0.0, weightDecay=1e-3,
                                            momentum=0.9)
    with _world1():
        p0, w_on, seen_on, opt = _train_distri(lars, True, CONST, L2)
        assert spy.calls == 3
        assert all(s["unpacked"] for s in seen_on), seen_on
        assert all(m.grad_clip is None for m in opt.optim_methods.values())
        _, w_off, _, _ = _train_distri(lars, False, CONST, L2)
        assert spy.calls == 6
    assert not torch.equal(w_on, _flat(p0))
    assert torch.equal(w_on, w_off)
