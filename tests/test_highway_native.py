"""The Highway kernels (ops/csrc/highway.hip) and the native path of ``Highway`` against the layer's equations in
plain torch fp64 on the host, on operands rounded to bf16 exactly as the device holds them:
``a = x@w.T + b; t = σ(a[:, :N]); h = act(a[:, N:]); y = t*h + (1-t)*x``, ``DG = [gy(h−x)t(1−t) | gy·t·act'(h)]``,
``gx = DG@w + gy(1−t)``, ``gW = DG.T@x``, ``gb = DG.sum(0)``.  The backward is teacher-forced: DG is computed from
the device's own bf16 gates, gx / gW / gb from the device's own bf16 DG, so a ReLU pre-activation within rounding
of zero or a bf16 tie in DG cannot flip a whole term of the next stage.

CPU part: the oracle matches ``Highway(...).to(float64)`` to 1e-12.  The bounds are those of
tests/test_rnn_oracle.py: bf16 outputs 2^-8·|ref| + A·rms(ref), fp32-held outputs A·rms(ref), A = 2e-5.  A stands
because this oracle in torch fp32 against itself in fp64, at every N × B × activation below, stays below 1e-5·rms
(test_oracle_fp32_error; worst observed 2.5e-6).

GPU part: the three ops at every N × B × activation, outputs in guarded buffers, all bit-equal over two runs; then
the layer with ``bigdl.highway.native`` on and off: fallback accounting, the native error at most max(2 × the
torch device path's error, 2^-8·max|ref|), accumulation over a second backward, inference bit-equal to training,
the same with ``with_bias=False``, and the three ineligible cases, which take the torch path and are counted.

Sizes the kernels use, and where N lies: batch tile 32 = two 16-row fragments (B 1 and 17 below, 70 across);
output-column tile 64 of forward and backward and the 16 columns of a wave (8 below a wave, 24 and 32 below the
tile, 64 on it, 128 on two, 200 across); reduction chunk 128 of the forward and N tile 128 of the weight gradient
(8 .. 64 below, 128 on it, 200 across); reduction chunk 64 of the backward over 2N and the weight gradient's tile
of 64 gate columns (2N = 16, 48 below, N = 32 on it, 64 and 128 on a multiple, 400 across; the gate / candidate
seam falls inside a chunk for N = 8, 24, 200).  The issue's 72 became 32 and 64 so that one size lies on each.
"""
import pytest
import torch

from test_rnn_oracle import Draw, Guard, NO, close_bf16, close_f32, d, dev  # noqa: F401

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64

NS = (8, 24, 32, 64, 128, 200)
BS = (1, 17, 70)
ACT = {"identity": lambda v: v, "tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid}
DACT = {"identity": torch.ones_like, "tanh": lambda h: 1 - h * h, "relu": lambda h: (h > 0).to(h.dtype),
        "sigmoid": lambda h: h * (1 - h)}


# ------------------------------------------------------------------------------------------ the oracle
def hw_fwd(x, w, b, act):
    """→ y, gates [t | h]."""
    N = x.shape[1]
    a = x @ w.T + b
    t, h = torch.sigmoid(a[:, :N]), ACT[act](a[:, N:])
    return t * h + (1 - t) * x, torch.cat((t, h), 1)


def hw_dg(gy, x, gates, act):
    N = x.shape[1]
    t, h = gates[:, :N], gates[:, N:]
    return torch.cat((gy * (h - x) * t * (1 - t), gy * t * DACT[act](h)), 1)


def hw_bwd(gy, x, gates, w, dg):
    """→ gx, gW, gb."""
    return dg @ w + gy * (1 - gates[:, :x.shape[1]]), dg.T @ x, dg.sum(0)


def hw_all(x, w, b, gy, act):
    """Un-forced: → y, gates, DG, gx, gW, gb."""
    y, gates = hw_fwd(x, w, b, act)
    dg = hw_dg(gy, x, gates, act)
    return (y, gates, dg, *hw_bwd(gy, x, gates, w, dg))


def draw(N, B, seed=0):
    r = Draw(seed)
    return r.n(B, N), r.n(2 * N, N, scale=N ** -0.5), r.n(2 * N, dt=f32), r.n(B, N)


def _layer(N, w, b, act, with_bias=True):
    from bigdl.nn import Highway
    m = Highway(N, with_bias=with_bias, activation=None if act == "identity" else act)
    m.weight.copy_(w)
    if with_bias:
        m.bias.copy_(b.to(bf))   # a bias both paths hold exactly
    return m


def _layer_run(m, x, gy):
    """→ y, gx, gradWeight, gradBias (None without a bias)."""
    y = m.forward(x)
    return y, m.backward(x, gy), m.gradWeight, getattr(m, "gradBias", None)


@pytest.mark.parametrize("act,with_bias", [(a, True) for a in ACT] + [("tanh", False)])
def test_oracle_matches_fp64_layer(act, with_bias):
    x, w, b, gy = (t.double() for t in draw(24, 3))
    b = b.to(bf).double() if with_bias else torch.zeros_like(b)
    m = _layer(24, w, b, act, with_bias).to(dtype=f64)
    m.zeroGradParameters()
    y, _, _, gx, gw, gb = hw_all(x, w, b, gy, act)
    for nm, a, r in zip(("y", "gx", "gW", "gb"), _layer_run(m, x, gy), (y, gx, gw, gb) if with_bias else (y, gx, gw)):
        assert float((a - r).abs().max()) <= 1e-12, nm


def test_oracle_fp32_error():
    worst = 0.0
    for N in NS:
        for B in BS:
            for act in ACT:
                v = draw(N, B)
                for lo, hi in zip(hw_all(*(t.float() for t in v), act), hw_all(*(t.double() for t in v), act)):
                    worst = max(worst, float((lo.double() - hi).abs().max() / hi.pow(2).mean().sqrt()))
    print(f"[highway] part=cpu what=fp32-vs-fp64 worst={worst:.3e}")
    assert worst < 1e-5, worst


# ------------------------------------------------------------------------------------------ the ops
@pytest.mark.gpu
@pytest.mark.parametrize("act", ACT)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_ops(NO, N, B, act):
    x, w, b, gy = draw(N, B)
    X, Wt, Bi, GY = dev(x), dev(w), dev(b), dev(gy)
    g, runs, tag = Guard(), [], f"{N}:B{B}:{act}"
    for _ in range(2):
        gates = g.new((B, 2 * N), bf)
        y = NO.highway_forward(X, Wt, Bi, act, gates=gates, out=g.new((B, N), bf))
        gx, dg = NO.highway_backward(GY, X, gates, Wt, act, out=g.new((B, N), bf), out_dg=g.new((B, 2 * N), bf))
        gb = g.new((2 * N,), f32)
        gw = NO.highway_wgrad(dg, X, out=g.new((2 * N, N), f32), out_bias=gb)
        runs.append((y, gates, dg, gx, gw, gb))
    gw3 = NO.highway_wgrad(dg, X, scale=-0.375, out=g.new((2 * N, N), f32))
    gx_keep = g.new((B, N), bf, init=gx)
    none, dg2 = NO.highway_backward(GY, X, gates, None, act, need_input=False, out=gx_keep, out_dg=g.new((B, 2 * N), bf))
    y_nb = NO.highway_forward(X, Wt, None, act, out=g.new((B, N), bf))   # no bias: a null pointer, inference form
    g.check()
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    assert none is None and torch.equal(dg2, dg) and torch.equal(gx_keep, gx)
    want_y, want_g = hw_fwd(d(x), d(w), d(b), act)
    want_dg = hw_dg(d(gy), d(x), d(gates), act)
    want_gx, want_gw, want_gb = hw_bwd(d(gy), d(x), d(gates), d(w), d(dg))
    close_bf16("highway", f"{tag}:y", y, want_y)
    close_bf16("highway", f"{tag}:gates", gates, want_g)
    close_bf16("highway", f"{tag}:DG", dg, want_dg)
    close_bf16("highway", f"{tag}:gx", gx, want_gx)
    close_f32("highway", f"{tag}:gW", gw, want_gw)
    close_f32("highway", f"{tag}:gW-scaled", gw3, -0.375 * want_gw)
    close_f32("highway", f"{tag}:gb", gb, want_gb)
    close_bf16("highway", f"{tag}:y-nobias", y_nb, hw_fwd(d(x), d(w), 0.0, act)[0])


# ------------------------------------------------------------------------------------------ the layer
def _bigdl():
    from bigdl import ops
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    return ops, config


def _device_runs(N, with_bias, natives, seed=1):
    """The device layer (tanh) with the property at each of ``natives`` → {native: [y, gx, gW, gb]}, the fp64
    oracle's results, the device layer and its inputs."""
    ops, config = _bigdl()
    x, w, b, gy = draw(N, 17, seed=seed)
    b = b.to(bf) if with_bias else torch.zeros_like(b)
    gpu = _layer(N, w, b, "tanh", with_bias).to(device="cuda")
    y, _, _, gx, gw, gb = hw_all(d(x), d(w), d(b), d(gy), "tanh")
    args, res = (x.cuda(), gy.cuda()), {}
    for native in natives:
        config.set_property("bigdl.highway.native", native)
        try:
            gpu.zeroGradParameters()
            ops.reset_fallbacks()
            res[native] = [t.clone() for t in _layer_run(gpu, *args) if t is not None]
            assert {k[:2] for k in ops.fallback_counts()} == (set() if native else {("highway", "disabled")})
        finally:
            config.set_property("bigdl.highway.native", True)
            ops.reset_fallbacks()
    return res, (y, gx, gw, gb), gpu, args


@pytest.mark.gpu
@pytest.mark.parametrize("N,with_bias", [(24, True), (200, True), (24, False)])
def test_layer_native_vs_fp64(N, with_bias):
    res, want, gpu, args = _device_runs(N, with_bias, (False, True))
    assert len(res[True]) == (4 if with_bias else 3)
    for nm, nat, tor, r in zip(("y", "gx", "gW", "gb"), res[True], res[False], want):
        e_nat, e_tor = float((d(nat) - r).abs().max()), float((d(tor) - r).abs().max())
        bound = max(2 * e_tor, 2.0 ** -8 * float(r.abs().max()))
        print(f"[highway] part=layer what={N}{'' if with_bias else '-nobias'}:{nm} native={e_nat:.3e} torch={e_tor:.3e} "
              f"frac={e_nat / bound:.3e}")
        assert e_nat <= bound, (nm, e_nat, e_tor)
    # a second backward accumulates (an overwrite would miss by max|one|); inference gives the training bits
    _layer_run(gpu, *args)
    for acc, one in zip((gpu.gradWeight, getattr(gpu, "gradBias", None)), res[True][2:]):
        assert float((acc - 2 * one).abs().max()) <= 1e-3 * float(one.abs().max())
    gpu.evaluate()
    assert torch.equal(gpu.forward(args[0]), res[True][0])


@pytest.mark.gpu
@pytest.mark.parametrize("why", ("geometry", "shape", "activation"))
def test_ineligible_takes_torch_path(why):
    """N = 12, a 1-D input and an activation outside the layer's table are counted and give what the property
    off gives: the torch path's bits, or for the 1-D input the torch path's error (its ``y[:, :size]``)."""
    ops, config = _bigdl()
    from bigdl.nn import ELU, Highway
    from bigdl.nn.abstractnn import LayerException
    N = 12 if why == "geometry" else 24
    x, w, b, _ = draw(N, 17, seed=2)
    gpu = _layer(N, w, b, "tanh").to(device="cuda") if why != "activation" else Highway(N, activation=ELU()).to(device="cuda")
    xin, got = (x[0] if why == "shape" else x).cuda(), {}
    for native in (True, False):
        config.set_property("bigdl.highway.native", native)
        ops.reset_fallbacks()
        try:
            got[native] = gpu.forward(xin)
        except LayerException as e:
            got[native] = type(e.__cause__)
        finally:
            counted = [k[:2] for k in ops.fallback_counts()]
            config.set_property("bigdl.highway.native", True)
            ops.reset_fallbacks()
        assert counted == [("highway", why if native else "disabled")]
    if why == "shape":   # both arms end in the torch code's IndexError, neither returns
        assert got[True] is IndexError and got[False] is IndexError, got
    else:
        assert torch.equal(got[True], got[False])
