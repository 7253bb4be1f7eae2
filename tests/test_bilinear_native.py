"""The Bilinear kernels (ops/csrc/bilinear.hip) and the native path of ``Bilinear`` against the layer's equation in
plain torch fp64 on the host: ``einsum("bi,kij,bj->bk") + b``, its three adjoint einsums and ``gy.sum(0)``, on
operands rounded to bf16 exactly as the device holds them.

CPU part: the oracle matches ``Bilinear(...).to(float64)`` to 1e-12.  The bounds are those of
tests/test_rnn_oracle.py: bf16 outputs 2^-8·|ref| + A·rms(ref), fp32-held outputs A·rms(ref), A = 2e-5.  A stands
because this oracle in torch fp32 against itself in fp64, at every geometry × B below, stays below
1e-5·rms (test_oracle_fp32_error; worst observed 3.6e-6).

GPU part: the three ops at every geometry × B in (1, 17, 70), outputs in guarded buffers, y / gx1 / gx2 / gW
bit-equal over two runs; then the layer with ``bigdl.bilinear.native`` on and off: fallback accounting, the native
error at most max(2 × the torch device path's error, 2^-8·max|ref|), accumulation over a second backward,
inference bit-equal to training, ``bias_res=False``, and an input size that is no multiple of 8.

Sizes the kernels use, and where the geometries lie: batch tile 32 = two 16-row fragments (B 1 and 17 below, 70
across); J chunk 128 of forward / gx1 and J tile 128 of the weight gradient (8, 40 below, 136, 264 across, 128
on it); I slab 16 per wave, 64 per round of the forward's four waves (8 below, 24, 72, 200 across, 128 on it);
I chunk and I tile 64 of gx2 and the weight gradient (8, 24 below, 72, 200 across, 128 on it); J tile 64 of gx2
(8, 40 below, 136, 264 across, 128 on it); k in rounds of four waves in gx1 (1, 2, 3 below, 5, 7 across, 4 on
it).  The issue's (128, 64, 2) is (128, 128, 2) here so that one size lies exactly on the 128-wide J chunk.
"""
import pytest
import torch

from test_rnn_oracle import Draw, Guard, NO, close_bf16, close_f32, d, dev  # noqa: F401

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64

GEOMS = ((8, 8, 1), (24, 40, 3), (72, 136, 5), (128, 128, 2), (200, 8, 7), (8, 264, 4))   # (I, J, K)
BS = (1, 17, 70)


# ------------------------------------------------------------------------------------------ the oracle
def bil_fwd(x1, x2, w, b):
    return torch.einsum("bi,kij,bj->bk", x1, w, x2) + b


def bil_bwd(x1, x2, w, gy):
    """→ gx1, gx2, gW, gb."""
    return (torch.einsum("bk,kij,bj->bi", gy, w, x2), torch.einsum("bk,kij,bi->bj", gy, w, x1),
            torch.einsum("bk,bi,bj->kij", gy, x1, x2), gy.sum(0))


def draw(geom, B, seed=0):
    I, J, K = geom
    r = Draw(seed)
    return r.n(B, I), r.n(B, J), r.n(K, I, J, scale=(I * J) ** -0.5), r.n(K, dt=f32), r.n(B, K)


def _layer_run(m, x1, x2, gy):
    """→ y, gx1, gx2, gradWeight, gradBias (None without a bias)."""
    from bigdl.utils.table import Table
    x = Table(x1, x2)
    y = m.forward(x)
    gx = m.backward(x, gy)
    return y, gx[1], gx[2], m.gradWeight, getattr(m, "gradBias", None)


def _layer(geom, w, b, bias_res=True):
    from bigdl.nn import Bilinear
    m = Bilinear(*geom, bias_res=bias_res)
    m.weight.copy_(w)
    if bias_res:
        m.bias.copy_(b.to(bf))   # a bias both paths hold exactly
    return m


@pytest.mark.parametrize("geom,bias_res", [(g, True) for g in GEOMS] + [((24, 40, 3), False)])
def test_oracle_matches_fp64_layer(geom, bias_res):
    x1, x2, w, b, gy = (t.double() for t in draw(geom, 3))
    b = b.to(bf).double() if bias_res else torch.zeros_like(b)
    m = _layer(geom, w, b, bias_res).to(dtype=f64)
    m.zeroGradParameters()
    got = _layer_run(m, x1, x2, gy)
    want = (bil_fwd(x1, x2, w, b), *bil_bwd(x1, x2, w, gy))
    for nm, a, r in zip(("y", "gx1", "gx2", "gW", "gb"), got, want if bias_res else want[:4]):
        assert float((a - r).abs().max()) <= 1e-12, nm


def test_oracle_fp32_error():
    worst = 0.0
    for geom in GEOMS:
        for B in BS:
            x1, x2, w, b, gy = draw(geom, B)
            run = lambda dt: (bil_fwd(x1.to(dt), x2.to(dt), w.to(dt), b.to(dt)),  # noqa: E731
                              *bil_bwd(x1.to(dt), x2.to(dt), w.to(dt), gy.to(dt)))
            for lo, hi in zip(run(f32), run(f64)):
                worst = max(worst, float((lo.double() - hi).abs().max() / hi.pow(2).mean().sqrt()))
    print(f"[bilinear] part=cpu what=fp32-vs-fp64 worst={worst:.3e}")
    assert worst < 1e-5, worst


# ------------------------------------------------------------------------------------------ the ops
@pytest.mark.gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "-".join(map(str, g)))
def test_ops(NO, geom, B):
    I, J, K = geom
    x1, x2, w, b, gy = draw(geom, B)
    want = (bil_fwd(d(x1), d(x2), d(w), d(b)), *bil_bwd(d(x1), d(x2), d(w), d(gy)))
    X1, X2, Wt, Bi, GY = dev(x1), dev(x2), dev(w), dev(b), dev(gy)
    g, runs, tag = Guard(), [], f"{I}-{J}-{K}:B{B}"
    for _ in range(2):
        y = NO.bilinear_forward(X1, X2, Wt, Bi, out=g.new((B, K), bf))
        gx1 = NO.bilinear_gx(1, GY, X2, Wt, out=g.new((B, I), bf))
        gx2 = NO.bilinear_gx(2, GY, X1, Wt, out=g.new((B, J), bf))
        gb = g.new((K,), f32)
        gw = NO.bilinear_wgrad(GY, X1, X2, out=g.new((K, I, J), f32), out_bias=gb)
        runs.append((y, gx1, gx2, gw))
    gw3 = NO.bilinear_wgrad(GY, X1, X2, scale=-0.375, out=g.new((K, I, J), f32))
    g.check()
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    close_bf16("bilinear", f"{tag}:y", y, want[0])
    close_bf16("bilinear", f"{tag}:gx1", gx1, want[1])
    close_bf16("bilinear", f"{tag}:gx2", gx2, want[2])
    close_f32("bilinear", f"{tag}:gW", gw, want[3])
    close_f32("bilinear", f"{tag}:gW-scaled", gw3, -0.375 * want[3])
    close_f32("bilinear", f"{tag}:gb", gb, want[4])
    # no bias: a null pointer
    close_bf16("bilinear", f"{tag}:y-nobias", NO.bilinear_forward(X1, X2, Wt), want[0] - d(b))


# ------------------------------------------------------------------------------------------ the layer
def _bigdl():
    from bigdl import ops
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    return ops, config


def _device_runs(geom, bias_res, natives, seed=1):
    """The device layer with the property at each of ``natives`` → {native: [y, gx1, gx2, gW, gb]}, the fp64
    layer's results, the device layer and its inputs."""
    ops, config = _bigdl()
    x1, x2, w, b, gy = draw(geom, 17, seed=seed)
    ref = _layer(geom, w, b, bias_res)
    gpu = ref.cloneModule().to(device="cuda")
    ref = ref.to(dtype=f64)
    ref.zeroGradParameters()
    want = _layer_run(ref, x1.double(), x2.double(), gy.double())
    args, res = (x1.cuda(), x2.cuda(), gy.cuda()), {}
    for native in natives:
        config.set_property("bigdl.bilinear.native", native)
        try:
            gpu.zeroGradParameters()
            ops.reset_fallbacks()
            res[native] = [t.clone() for t in _layer_run(gpu, *args) if t is not None]
            assert {k[:2] for k in ops.fallback_counts()} == (set() if native else {("bilinear", "disabled")})
        finally:
            config.set_property("bigdl.bilinear.native", True)
            ops.reset_fallbacks()
    return res, want, gpu, args


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(24, 40, 3), (72, 136, 5)], ids=lambda g: "-".join(map(str, g)))
def test_layer_native_vs_fp64(geom):
    res, want, gpu, args = _device_runs(geom, True, (False, True))
    for nm, nat, tor, r in zip(("y", "gx1", "gx2", "gW", "gb"), res[True], res[False], want):
        e_nat, e_tor = float((d(nat) - r).abs().max()), float((d(tor) - r).abs().max())
        bound = max(2 * e_tor, 2.0 ** -8 * float(r.abs().max()))
        print(f"[bilinear] part=layer what={'-'.join(map(str, geom))}:{nm} native={e_nat:.3e} torch={e_tor:.3e} "
              f"frac={e_nat / bound:.3e}")
        assert e_nat <= bound, (nm, e_nat, e_tor)
    # a second backward accumulates (an overwrite would miss by max|one|); inference gives the training bits
    _layer_run(gpu, *args)
    for acc, one in ((gpu.gradWeight, res[True][3]), (gpu.gradBias, res[True][4])):
        assert float((acc - 2 * one).abs().max()) <= 1e-3 * float(one.abs().max())
    gpu.evaluate()
    from bigdl.utils.table import Table
    assert torch.equal(gpu.forward(Table(args[0], args[1])), res[True][0])


@pytest.mark.gpu
def test_layer_without_bias():
    res, want, gpu, _ = _device_runs((24, 40, 3), False, (True,))
    assert len(res[True]) == 4
    for nm, nat, r in zip(("y", "gx1", "gx2", "gW"), res[True], want):
        (close_f32 if nm == "gW" else close_bf16)("bilinear", f"nobias:{nm}", nat, r)


@pytest.mark.gpu
@pytest.mark.parametrize("geom,why", [((24, 40, 3), "disabled"), ((12, 40, 3), "geometry")])
def test_ineligible_takes_torch_path(geom, why):
    ops, config = _bigdl()
    from bigdl.utils.table import Table
    x1, x2, w, b, gy = draw(geom, 17, seed=2)
    gpu = _layer(geom, w, b).to(device="cuda")
    config.set_property("bigdl.bilinear.native", why != "disabled")
    ops.reset_fallbacks()
    try:
        y = gpu.forward(Table(x1.cuda(), x2.cuda()))
        assert [k[:2] for k in ops.fallback_counts()] == [("bilinear", why)]
    finally:
        config.set_property("bigdl.bilinear.native", True)
        ops.reset_fallbacks()
    # the torch path rounds an intermediate z and y to bf16: at worst 2^-9·(Σ|z·x| + |y|); with these draws rms(y) is
    # 1, Σ|z·x| ≈ 0.64·√(I or J) ≤ 4.1 and max|ref| ≥ 2, so 3·2^-8·max|ref| covers it without leaning on the result
    ref = bil_fwd(d(x1), d(x2), d(w), d(b.to(bf)))
    err = float((d(y) - ref).abs().max())
    print(f"[bilinear] part=layer what=fallback-{why}:y err={err:.3e} max|ref|={float(ref.abs().max()):.3e}")
    assert err <= 3 * 2.0 ** -8 * float(ref.abs().max())
