"""The locally connected kernels (ops/csrc/locally_connected.hip) and the native path of LocallyConnected2D / 1D
against the layer's equation in plain torch fp64 on the host: unfold + einsum, and its hand-written adjoint
(fold, two einsums, a sum), on operands rounded to bf16 exactly as the device holds them.

CPU part: the oracle matches ``LocallyConnected2D/1D(...).to(float64)`` to 1e-12.  The bounds are those of
tests/test_rnn_oracle.py: bf16 outputs 2^-8·|ref| + A·rms(ref), fp32-held outputs A·rms(ref), A = 2e-5.  A
stands because this oracle in torch fp32 against itself in fp64, at every geometry below with N = 70 (K up to
576 forward, 648 in the data gradient), is worst 1.4e-6·rms, below 1e-5 (test_oracle_fp32_error).

GPU part: the four ops at every geometry × N in (1, 17, 70), outputs in guarded buffers, forward / gx / gW
bit-equal over two runs; then the layers with ``bigdl.lc.native`` on and off: fallback accounting, the
native error at most max(2 × the torch device path's error, 2^-8·max|ref|), accumulation over a second
backward, inference bit-equal to training.  The K chunk of the kernels is 128: K = 72 and 24 lie below it,
216, 200, 576 (and 360, 648, 144 in the data gradient) exceed it, and only 576 is a multiple of it.
"""
import pytest
import torch
import torch.nn.functional as F

from test_rnn_oracle import Draw, Guard, NO, close_bf16, close_f32, d, dev  # noqa: F401

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64

# (C, O, (kH, kW), (sH, sW), (pH, pW), (H, W)); the 1-D layer's (F, O, kW, stride, frames) is the image 1 × frames
GEOMS = {
    "2d-8-8-k3": (8, 8, (3, 3), (1, 1), (0, 0), (5, 6)),
    "2d-24-40-k3p1": (24, 40, (3, 3), (1, 1), (1, 1), (5, 6)),
    "2d-16-24-k2x3s2x1": (16, 24, (2, 3), (2, 1), (0, 1), (7, 6)),
    "2d-8-72-k5s2p2": (8, 72, (5, 5), (2, 2), (2, 2), (9, 9)),
    "2d-64-16-k3p1": (64, 16, (3, 3), (1, 1), (1, 1), (4, 4)),
    "1d-8-8-k3": (8, 8, (1, 3), (1, 1), (0, 0), (1, 9)),
    "1d-24-40-k4s2": (24, 40, (1, 4), (1, 2), (0, 0), (1, 11)),
}
NS = (1, 17, 70)


def geom_of(name):
    C, O, k, s, p, hw = GEOMS[name]
    return (*hw, C, O, *k, *s, *p), ("TC" if name.startswith("1d") else "CT")


# ------------------------------------------------------------------------------------------ the oracle
def _cols(x, geom, order):
    """x (N, H, W, C) → patches (N, K, L), K in the layer's order."""
    H, W, C, O, kH, kW, sH, sW, pH, pW = geom
    cols = F.unfold(x.permute(0, 3, 1, 2), (kH, kW), padding=(pH, pW), stride=(sH, sW))
    if order == "TC":
        cols = cols.view(len(x), C, kH * kW, -1).transpose(1, 2).reshape(len(x), C * kH * kW, -1)
    return cols


def lc_fwd(x, w, b, geom, order):
    """→ y (N, L, O)."""
    return torch.einsum("nkl,lok->nlo", _cols(x, geom, order), w) + b


def lc_bwd(x, w, gy, geom, order):
    """gy (N, L, O) → gx (N, H, W, C), gW (L, O, K), gb (L, O)."""
    H, W, C, O, kH, kW, sH, sW, pH, pW = geom
    gc = torch.einsum("nlo,lok->nkl", gy, w)
    if order == "TC":
        gc = gc.view(len(x), kH * kW, C, -1).transpose(1, 2).reshape(len(x), C * kH * kW, -1)
    gx = F.fold(gc, (H, W), (kH, kW), padding=(pH, pW), stride=(sH, sW)).permute(0, 2, 3, 1)
    return gx, torch.einsum("nlo,nkl->lok", gy, _cols(x, geom, order)), gy.sum(0)


def draw(name, N, seed=0):
    geom, order = geom_of(name)
    H, W, C, O, kH, kW, sH, sW, pH, pW = geom
    L, K = ((H + 2 * pH - kH) // sH + 1) * ((W + 2 * pW - kW) // sW + 1), C * kH * kW
    r = Draw(seed)
    return geom, order, r.n(N, H, W, C), r.n(L, O, K, scale=K ** -0.5), r.n(L, O, dt=f32), r.n(N, L, O)


def _layer(name, fmt="NCHW"):
    from bigdl.nn import LocallyConnected1D, LocallyConnected2D
    C, O, k, s, p, hw = GEOMS[name]
    if name.startswith("1d"):
        return LocallyConnected1D(hw[1], C, O, k[1], s[1])
    return LocallyConnected2D(C, hw[1], hw[0], O, k[1], k[0], s[1], s[0], p[1], p[0], data_format=fmt)


def _layer_fwd(m, name, fmt, x):
    """Oracle-shaped x (N, H, W, C) → the layer's input, its output as (N, oH, oW, O) (1-D: (N, L, O))."""
    if name.startswith("1d"):
        return x.squeeze(1), m.forward(x.squeeze(1))
    xin = x if fmt == "NHWC" else x.permute(0, 3, 1, 2)
    y = m.forward(xin)
    return xin, y if fmt == "NHWC" else y.permute(0, 2, 3, 1)


def _layer_run(m, name, fmt, x, gy):
    """→ y, gx (both in the oracle's shapes), gradWeight, gradBias."""
    xin, y = _layer_fwd(m, name, fmt, x)
    g = gy.view(y.shape)
    nchw = fmt == "NCHW" and not name.startswith("1d")
    gx = m.backward(xin, g.permute(0, 3, 1, 2) if nchw else g)
    return y.reshape(gy.shape), (gx.permute(0, 2, 3, 1) if nchw else gx).reshape(x.shape), m.gradWeight, m.gradBias


@pytest.mark.parametrize("name,fmt", [(n, "NCHW") for n in GEOMS] + [("2d-24-40-k3p1", "NHWC")])
def test_oracle_matches_fp64_layers(name, fmt):
    geom, order, x, w, b, gy = (t.double() if isinstance(t, torch.Tensor) else t for t in draw(name, 3))
    m = _layer(name, fmt).to(dtype=f64)
    m.weight.copy_(w), m.bias.copy_(b)
    m.zeroGradParameters()
    got = _layer_run(m, name, fmt, x, gy)
    for nm, a, r in zip(("y", "gx", "gW", "gb"), got, (lc_fwd(x, w, b, geom, order), *lc_bwd(x, w, gy, geom, order))):
        assert float((a - r).abs().max()) <= 1e-12, nm


def test_oracle_fp32_error():
    worst = 0.0
    for name in GEOMS:
        geom, order, x, w, b, gy = draw(name, max(NS))
        run = lambda dt: (lc_fwd(x.to(dt), w.to(dt), b.to(dt), geom, order),  # noqa: E731
                          *lc_bwd(x.to(dt), w.to(dt), gy.to(dt), geom, order))
        for lo, hi in zip(run(f32), run(f64)):
            worst = max(worst, float((lo.double() - hi).abs().max() / hi.pow(2).mean().sqrt()))
    print(f"[lc] part=cpu what=fp32-vs-fp64 worst={worst:.3e}")
    assert worst < 1e-5, worst


# ------------------------------------------------------------------------------------------ the ops
@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_ops(NO, name, N):
    geom, order, x, w, b, gy = draw(name, N)
    H, W, C, O = geom[:4]
    want_y = lc_fwd(d(x), d(w), d(b), geom, order)
    want = (want_y, *lc_bwd(d(x), d(w), d(gy), geom, order))
    X, Wt, B, GY = dev(x), dev(w), dev(b), dev(gy)
    g, runs = Guard(), []
    for _ in range(2):
        y = NO.lc_forward(X, Wt, B, geom, order, out=g.new(want_y.shape, bf))
        wd = NO.lc_weight_transpose(Wt, geom, order, out=g.new((NO.lc_wd_numel(geom),), bf))
        gx = NO.lc_dgrad(GY, wd, geom, N, out=g.new((N, H, W, C), bf))
        gw = NO.lc_wgrad(X, GY, geom, order, out=g.new(w.shape, f32))
        runs.append((y, gx, gw))
    gb = NO.colsum_acc(GY.view(N, -1), g.new((b.numel(),), f32, init=torch.zeros(b.numel()))).view(b.shape)
    g.check()
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    close_bf16("lc", f"{name}:N{N}:y", y, want[0])
    close_bf16("lc", f"{name}:N{N}:gx", gx, want[1])
    close_f32("lc", f"{name}:N{N}:gW", gw, want[2])
    close_f32("lc", f"{name}:N{N}:gb", gb, want[3])
    # no bias: a null pointer
    close_bf16("lc", f"{name}:N{N}:y-nobias", NO.lc_forward(X, Wt, None, geom, order).view(y.shape), want[0] - d(b))


# ------------------------------------------------------------------------------------------ the layers
def _bigdl():
    from bigdl import ops
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    return ops, config


@pytest.mark.gpu
@pytest.mark.parametrize("name,fmt", [("2d-24-40-k3p1", "NCHW"), ("2d-24-40-k3p1", "NHWC"), ("1d-24-40-k4s2", "NCHW")])
def test_layer_native_vs_fp64(name, fmt):
    ops, config = _bigdl()
    geom, order, x, w, b, gy = draw(name, 17, seed=1)
    ref = _layer(name, fmt)
    ref.weight.copy_(w), ref.bias.copy_(b.to(bf))
    gpu = ref.cloneModule().to(device="cuda")
    ref = ref.to(dtype=f64)
    ref.zeroGradParameters()
    want = _layer_run(ref, name, fmt, x.double(), gy.double())
    res = {}
    for native in (False, True):
        config.set_property("bigdl.lc.native", native)
        try:
            gpu.zeroGradParameters()
            ops.reset_fallbacks()
            res[native] = [t.clone() for t in _layer_run(gpu, name, fmt, x.cuda(), gy.cuda())]
            assert {k[0] for k in ops.fallback_counts()} == (set() if native else {"locally_connected"})
        finally:
            config.set_property("bigdl.lc.native", True)
    for nm, nat, tor, r in zip(("y", "gx", "gW", "gb"), res[True], res[False], want):
        e_nat, e_tor = float((d(nat) - r).abs().max()), float((d(tor) - r).abs().max())
        bound = max(2 * e_tor, 2.0 ** -8 * float(r.abs().max()))
        print(f"[lc] part=layer what={name}:{fmt}:{nm} native={e_nat:.3e} torch={e_tor:.3e} frac={e_nat / bound:.3e}")
        assert e_nat <= bound, (nm, e_nat, e_tor)
    # a second backward accumulates (an overwrite would miss by max|one|); inference gives the training bits
    y2 = _layer_run(gpu, name, fmt, x.cuda(), gy.cuda())[0]
    for acc, one in ((gpu.gradWeight, res[True][2]), (gpu.gradBias, res[True][3])):
        assert float((acc - 2 * one).abs().max()) <= 1e-3 * float(one.abs().max())
    gpu.evaluate()
    assert torch.equal(_layer_fwd(gpu, name, fmt, x.cuda())[1].reshape(y2.shape), res[True][0])


@pytest.mark.gpu
def test_ineligible_takes_torch_path():
    ops, config = _bigdl()
    from bigdl.nn import LocallyConnected2D
    m = LocallyConnected2D(3, 6, 5, 8, 3, 3).to(device="cuda")
    x = torch.randn(2, 3, 5, 6).to(bf).cuda()
    ops.reset_fallbacks()
    try:
        y = m.forward(x)
        assert [k[:2] for k in ops.fallback_counts()] == [("locally_connected", "channels")]
        with torch.no_grad():
            assert torch.equal(y, m._forward(x))
    finally:
        ops.reset_fallbacks()
