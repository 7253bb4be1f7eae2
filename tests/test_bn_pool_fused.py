"""BN (+ReLU) fused into the 3×3 / stride-2 max-pool, forward and backward (bigdl.fusion.bnpool).

Forward: ``bigdl_bn_maxpool_fwd`` applies bf16(relu(fma(x, scale, shift))) to every window tap on load
and compares the ROUNDED values, so the pooled tensor and the int8 argmax must be bit-identical to the
unfused native chain (BN apply → max-pool).  Backward: ``bigdl_bn_bwd_pool`` gathers the pool's input
gradient through the argmax while loading (summed in fp32) and recomputes the ReLU mask from the
forward coefficients; it is checked against an fp64 BN → ReLU → max-pool backward with the bounds
of tests/test_native_kernels.py::test_bn_train_fwd_bwd, and must be no less accurate than the unfused
native chain.  The mask options alone (recomputed / bits instead of y > 0) must not change a bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
K, S = (3, 3), (2, 2)
SHAPES = [(C, H, W, pad) for C in (8, 64) for (H, W) in ((7, 7), (8, 8), (9, 10)) for pad in (0, 1)]
# (the issue's shapes run one block per pass; this one spreads the backward over several)
BIG = (64, 41, 38, 1)


def _native():
    from bigdl.ops import native as N
    if not N.has("batchnorm_forward_train"):
        pytest.fail("native library not loaded")
    return N.native_ops


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _random_x(C, H, W, n=2):
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    x = torch.randn(n, C, H, W, generator=g) * 1.5 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    return _cl(x.to(dev).bfloat16()), gamma.to(dev), beta.to(dev)


LOW, ONE, ONE_UP = -9.0, 1.0, 1.0078125  # ONE_UP: the bf16 successor of 1.0


def _crafted_x(C, H, W):
    """Three input values only, LOW in a fraction f of the places (a quarter, plus the image corner: up to
    0.45 for the smallest image).  Normalised, a LOW is −sqrt((1 − f) / f) ≤ −1.1 and a ONE is
    sqrt(f / (1 − f)) ≥ 0.57, so with β = γ / 2 a LOW becomes ≤ −0.6 γ (windows of LOW are all ≤ 0 after
    the ReLU; the image corner is one) and a ONE ≥ 1.07 γ.  Equal inputs give equal positive maxima.
    ONE and ONE_UP differ by one bf16 ulp: their fp32 BN outputs differ by ≈ 0.0018 γ, under half a
    bf16 ulp of the output, so in most channels they round to the same bf16."""
    g = torch.Generator().manual_seed(77 + C + H)
    pick = torch.randint(0, 4, (2, C, H, W), generator=g)
    x = torch.full((2, C, H, W), LOW)
    x[pick == 1] = ONE
    x[pick == 2] = ONE_UP
    x[pick == 3] = ONE
    x[0, :, :4, :4] = LOW
    gamma = 0.02 + 0.01 * torch.arange(C, dtype=torch.float32)
    beta = 0.5 * gamma
    return _cl(x.to(dev).bfloat16()), gamma.to(dev), beta.to(dev)


_CACHE = {}


def _case(kind, C, H, W, pad):
    """Inputs, the native BN forward (statistics, coefficients, dense y) and both pooled results, computed
    once per case and shared by the forward and backward tests (never modified)."""
    key = (kind, C, H, W, pad)
    if key in _CACHE:
        return _CACHE[key]
    N = _native()
    from bigdl.ops.reference import BNOut
    x, gamma, beta = (_crafted_x if kind == "crafted" else _random_x)(C, H, W)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    coef = torch.empty(2 * C, device=dev)
    r = N.batchnorm_forward_train(x, gamma, beta, rm, rv, 0.1, 1e-5, relu=True, coef_out=coef)
    assert r is not NotImplemented
    y, mean, invstd = r
    r = N.maxpool2d_forward(y, K, S, (pad, pad), False)
    assert r is not NotImplemented
    yp, idx = r
    r = N.bn_maxpool_forward(BNOut(x, coef, relu=True), K, S, (pad, pad), False)
    assert r is not NotImplemented
    fp, fidx = r
    g = torch.Generator().manual_seed(5)
    gp = _cl(torch.randn(yp.shape, generator=g).to(dev).bfloat16())
    d = dict(x=x, gamma=gamma, beta=beta, coef=coef, y=y, mean=mean, invstd=invstd, yp=yp, idx=idx, fp=fp, fidx=fidx,
             gp=gp, pad=pad)
    _CACHE[key] = d
    return d


def _windows(t, pad):
    """[N][C][9][P·Q] window taps of an NCHW tensor (out-of-image taps −inf)."""
    n, c = t.shape[:2]
    tp = torch.nn.functional.pad(t.float(), (pad, pad, pad, pad), value=float("-inf"))
    return torch.nn.functional.unfold(tp, 3, stride=2).view(n, c, 9, -1)


@pytest.mark.parametrize("C,H,W,pad", SHAPES + [BIG])
@pytest.mark.parametrize("kind", ["random", "crafted"])
def test_forward_bit_identical(kind, C, H, W, pad):
    d = _case(kind, C, H, W, pad)
    torch.testing.assert_close(d["fp"], d["yp"], rtol=0, atol=0)
    assert torch.equal(d["fidx"].t, d["idx"].t)
    # the form without argmax (idx == nullptr)
    N = _native()
    from bigdl.ops.reference import BNOut
    r = N.bn_maxpool_forward(BNOut(d["x"], d["coef"], relu=True), K, S, (pad, pad), False, need_indices=False)
    assert r is not NotImplemented and r[1] is None
    torch.testing.assert_close(r[0], d["yp"], rtol=0, atol=0)


@pytest.mark.parametrize("C,H,W,pad", [(8, 8, 8, 1), (64, 9, 10, 0), (64, 9, 10, 1)])
def test_crafted_input_has_the_edge_cases(C, H, W, pad):
    """The crafted tensor really contains what it is meant to (checked on the unfused native y)."""
    d = _case("crafted", C, H, W, pad)
    wy, wx = _windows(d["y"], pad), _windows(d["x"], pad)
    top = wy.max(dim=2, keepdim=True).values
    assert bool((top <= 0).any()), "no window that is all <= 0 after BN + ReLU"
    at_top = (wy == top) & (top > 0)
    assert bool((at_top.sum(2) >= 2).any()), "no window with several equal positive maxima"
    x_hi = torch.where(at_top, wx, torch.full_like(wx, float("-inf"))).max(2).values
    x_lo = torch.where(at_top, wx, torch.full_like(wx, float("inf"))).min(2).values
    assert bool(((at_top.sum(2) >= 2) & (x_hi > x_lo)).any()), \
        "no window whose equal bf16 maxima come from different inputs (different fp32 BN outputs)"


def test_forward_rejects_other_geometry():
    N = _native()
    from bigdl.ops import native
    from bigdl.ops.reference import BNOut
    d = _case("random", 8, 8, 8, 1)
    b = BNOut(d["x"], d["coef"], relu=True)
    assert N.bn_maxpool_forward(b, (2, 2), S, (0, 0), False) is NotImplemented
    assert N.bn_maxpool_forward(b, K, (1, 1), (1, 1), False) is NotImplemented
    assert N.bn_maxpool_forward(b, K, S, (1, 1), True) is NotImplemented
    x, y = d["x"], torch.empty_like(d["fp"])
    rc = native.lib().bigdl_bn_maxpool_fwd(native.ptr(x), native.ptr(d["coef"]), native.ptr(y), None, 2, 8, 8, 8, 4, 4,
                                           3, 3, 1, 1, 1, 1, 1, None)
    assert rc != 0  # hipErrorInvalidValue: stride 1 is not the k3s2 geometry
    rc = native.lib().bigdl_bn_maxpool_fwd(native.ptr(x), native.ptr(d["coef"]), native.ptr(y), None, 2, 8, 8, 12, 4, 4,
                                           3, 3, 2, 2, 1, 1, 1, None)
    assert rc != 0  # C % 8 != 0


def _dense_pool_grad64(gp, idx, H, W, pad):
    """fp64 max-pool backward through the forward's int8 argmax (the selection the backward is defined by)."""
    n, c, P, Q = gp.shape
    canvas = torch.zeros(n, c, H + 2 * pad + 2, W + 2 * pad + 2, dtype=torch.float64, device=gp.device)
    arg = idx.permute(0, 3, 1, 2).to(torch.int64)  # [N][C][P][Q]
    g64 = gp.double()
    for k in range(9):
        i, j = divmod(k, 3)
        canvas[:, :, i:i + 2 * P:2, j:j + 2 * Q:2] += torch.where(arg == k, g64, torch.zeros_like(g64))
    return canvas[:, :, pad:pad + H, pad:pad + W]


def _backward_all(d):
    """(fused, unfused native chain, fp64 reference): each gx, dγ, dβ, folded conv-bias gradient."""
    if "bwd" in d:
        return d["bwd"]
    N = _native()
    from bigdl.ops import reference as R
    from bigdl.ops.reference import BNOut, PoolGrad
    x, gamma, mean, invstd, coef, y, gp, pad = (d[k] for k in ("x", "gamma", "mean", "invstd", "coef", "y", "gp", "pad"))
    C, H, W = x.shape[1:]
    p = (pad, pad)

    def acc():
        return [torch.zeros(C, device=dev) for _ in range(3)]
    # fused
    gg, gb, cb = acc()
    pg = PoolGrad(gp, d["fidx"], K, S, p, BNOut(x, coef, relu=True))
    gx = N.batchnorm_backward_pool(pg, x, gamma, mean, invstd, fcoef=coef, gg_acc=gg, gb_acc=gb, scale=1.0,
                                   cbias_acc=cb, cbias_scale=1.0)
    assert gx is not NotImplemented
    fused = (gx, gg, gb, cb)
    # the deferred gradient densified = today's pool backward
    gd = N.maxpool2d_backward(gp, y, d["idx"], K, S, p, False)
    assert gd is not NotImplemented
    torch.testing.assert_close(pg.dense(), gd, rtol=0, atol=0)
    # unfused native chain
    gg, gb, cb = acc()
    r = N.batchnorm_backward(gd, x, gamma, mean, invstd, y=y, relu=True, gg_acc=gg, gb_acc=gb, scale=1.0,
                             cbias_acc=cb, cbias_scale=1.0)
    assert r is not NotImplemented
    unfused = (r[0], gg, gb, cb)
    # fp64: batch statistics, BN, ReLU mask and the gather all in double
    x64, g64 = x.double(), gamma.double()
    dims = (0, 2, 3)
    m64 = x64.mean(dims)
    is64 = torch.rsqrt(x64.var(dims, unbiased=False) + 1e-5)
    y64 = torch.relu((x64 - m64.view(1, C, 1, 1)) * (is64 * g64).view(1, C, 1, 1) + d["beta"].double().view(1, C, 1, 1))
    gd64 = _dense_pool_grad64(gp, d["idx"].t, H, W, pad)
    gg, gb, cb = [torch.zeros(C, device=dev, dtype=torch.float64) for _ in range(3)]
    gx64, _ = R.batchnorm_backward(gd64, x64, g64, m64, is64, y=y64, relu=True, gg_acc=gg, gb_acc=gb, scale=1.0,
                                   cbias_acc=cb, cbias_scale=1.0)
    d["bwd"] = (fused, unfused, (gx64, gg, gb, cb))
    return d["bwd"]


@pytest.mark.parametrize("C,H,W,pad", SHAPES + [BIG])
@pytest.mark.parametrize("kind", ["random", "crafted"])
def test_backward_against_fp64(kind, C, H, W, pad):
    fused, unfused, ref = _backward_all(_case(kind, C, H, W, pad))
    err_f = float((fused[0].double() - ref[0]).abs().max())
    err_u = float((unfused[0].double() - ref[0]).abs().max())
    print(f"{kind} C={C} {H}x{W} pad={pad}: max |gx - fp64| fused {err_f:.6g} unfused {err_u:.6g}")
    torch.testing.assert_close(fused[3].double(), ref[3], rtol=0, atol=5e-2)
    torch.testing.assert_close(fused[1].double(), ref[1], rtol=2e-3, atol=2e-2)
    torch.testing.assert_close(fused[2].double(), ref[2], rtol=2e-3, atol=2e-2)
    torch.testing.assert_close(fused[0].double(), ref[0], rtol=3e-2, atol=3e-2)
    assert err_f <= err_u, (err_f, err_u)


@pytest.mark.parametrize("N_,C,H,W", [(2, 8, 7, 7), (2, 64, 9, 10), (4, 64, 24, 24), (2, 256, 6, 5)])
@pytest.mark.parametrize("gres", [False, True])
def test_mask_sources_change_no_bit(N_, C, H, W, gres):
    """Dense gradient, no pool: the recomputed mask and the mask bits against the y > 0 path."""
    N = _native()
    g = torch.Generator().manual_seed(3 * C + H)
    x = _cl((torch.randn(N_, C, H, W, generator=g) * 2 - 0.2).to(dev).bfloat16())
    gy = _cl(torch.randn(N_, C, H, W, generator=g).to(dev).bfloat16())
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.3).to(dev)
    coef = torch.empty(2 * C, device=dev)
    bits = torch.empty(x.numel() // 8, dtype=torch.uint8, device=dev)
    r = N.batchnorm_forward_train(x, gamma, beta, torch.zeros(C, device=dev), torch.ones(C, device=dev), 0.1, 1e-5,
                                  relu=True, coef_out=coef, bits_out=bits)
    assert r is not NotImplemented
    y, mean, invstd = r
    assert 0.2 < float((y > 0).float().mean()) < 0.8

    def run(**mask):
        acc = [torch.zeros(C, device=dev) for _ in range(3)]
        out = N.batchnorm_backward(gy, x, gamma, mean, invstd, relu=True, gg_acc=acc[0], gb_acc=acc[1], scale=0.5,
                                   cbias_acc=acc[2], cbias_scale=1.0, want_gres=gres, **mask)
        assert out is not NotImplemented
        return out, acc
    (gx0, gr0), acc0 = run(y=y)
    for mask in (dict(fcoef=coef), dict(mask_bits=bits)):
        (gx, gr), acc = run(**mask)
        assert torch.equal(gx, gx0), mask.keys()
        for a, a0 in zip(acc, acc0):  # dγ, dβ, the folded bias: the partial sums did not change
            torch.testing.assert_close(a, a0, rtol=0, atol=0)
        if gres:
            assert torch.equal(gr, gr0)


# ---------------------------------------------------------------------------------------------- module level
def _stem(seed=3):
    from bigdl.nn import Sequential, SpatialConvolution, SpatialBatchNormalization, ReLU, SpatialMaxPooling
    from bigdl.nn.fusion import fuse
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.utils.random import RNG
    config.set_property("bigdl.compute.dtype", "bf16")
    Engine.init(device="cuda:0")
    RNG.setSeed(seed)
    m = (Sequential().add(SpatialConvolution(16, 16, 3, 3, 1, 1, 1, 1)).add(SpatialBatchNormalization(16))
         .add(ReLU(True)).add(SpatialMaxPooling(3, 3, 2, 2, 1, 1)).add(SpatialConvolution(16, 32, 3, 3, 1, 1, 1, 1)))
    m.cuda()
    m.training()
    fuse(m)
    m.getParameters()
    m.flat_parameters().enable_shadow(torch.bfloat16)
    return m


def _step(m, x, gy, on, extra):
    from bigdl.utils import config
    for e, v in zip(m.getExtraParameter(), extra):  # the statistics shift is the running mean: same in both runs
        e.copy_(v)
    for mod in m.flattened_modules():
        mod.__dict__.pop("_kbuf", None)
    prev = config.get_property("bigdl.fusion.bnpool")
    config.set_property("bigdl.fusion.bnpool", on)
    try:
        m.zeroGradParameters()
        y = m.forward(x)
        bn_out = m.modules[1].output
        m.backward(x, gy)
        torch.cuda.synchronize()
    finally:
        config.set_property("bigdl.fusion.bnpool", prev)
    return y.clone(), [g.float().clone() for g in m.parameters()[1]], bn_out


def test_module_step_fused_equals_unfused():
    from bigdl.ops.reference import BNOut, BNPoolOut
    m = _stem()
    g = torch.Generator().manual_seed(0)
    # (small on purpose: dγ / dβ of the UNFUSED run carry its bf16 rounding of the gathered pool gradient,
    # an error that grows with sqrt(N·H·W) while the project's bound for them is absolute)
    x = _cl(torch.randn(2, 16, 9, 10, generator=g).cuda().bfloat16())
    y0 = m.forward(x)
    gy = torch.randn(y0.shape, generator=g).cuda().to(y0.dtype)
    extra = [e.clone() for e in m.getExtraParameter()]
    ya, pa, oa = _step(m, x, gy, False, extra)
    yb, pb, ob = _step(m, x, gy, True, extra)
    # the fused run never wrote the BN output; its deferred form is the pool's own type, not the block tails'
    assert isinstance(oa, torch.Tensor) and isinstance(ob, BNPoolOut) and not isinstance(ob, BNOut)
    torch.testing.assert_close(yb, ya, rtol=0, atol=0)
    names = ("conv1.w", "conv1.b", "bn.w", "bn.b", "conv2.w", "conv2.b")
    assert len(pa) == len(pb) == 6
    for n, u, v in zip(names, pb, pa):
        rel = float((u - v).norm() / v.norm().clamp_min(1e-12))
        print(f"{n}: |v| max {float(v.abs().max()):.4g}, max |u - v| {float((u - v).abs().max()):.4g}, "
              f"||u - v|| / ||v|| {rel:.3g}")
        if n in ("bn.w", "bn.b"):
            torch.testing.assert_close(u, v, rtol=2e-3, atol=2e-2, msg=lambda s, n=n: f"{n}: {s}")
        elif n == "conv1.b":  # folded into the BN: the closed-form bias gradient
            torch.testing.assert_close(u, v, rtol=0, atol=5e-2, msg=lambda s, n=n: f"{n}: {s}")
        elif n.startswith("conv2"):  # downstream of the pool: same inputs, same kernels
            torch.testing.assert_close(u, v, rtol=0, atol=0, msg=lambda s, n=n: f"{n}: {s}")
        else:
            # conv1's weight gradient sums x · gx over all N·H·W pixels, so the element bounds of gx do not
            # carry over.  The two runs' gx are bf16 roundings (2^-9 relative each) of values that differ
            # only by the unfused path's extra bf16 rounding of the gathered pool gradient (2^-9 again):
            # ||Δgx|| ≤ 3 · 2^-9 ||gx||, and the sum over pixels does not amplify a relative perturbation
            # of its incoherent part — the same bound in the norm
            assert rel <= 3 * 2.0 ** -9, (n, rel)


def test_second_reader_of_the_deferred_output_gets_it_dense():
    """Anything but the pool that reads the BN's deferred output builds it (BNOut.dense), and a deferred
    pool gradient that does not reach the BN that deferred is built by the plain pool backward."""
    from bigdl.nn import SpatialConvolution
    from bigdl.ops.reference import BNOut, BNPoolOut, PoolGrad
    from bigdl.utils import config
    m = _stem(seed=4)
    side = SpatialConvolution(16, 8, 1, 1)
    side.cuda()
    side.training()
    g = torch.Generator().manual_seed(1)
    x = _cl(torch.randn(2, 16, 9, 10, generator=g).cuda().bfloat16())
    extra = [e.clone() for e in m.getExtraParameter()]
    gy = torch.randn(m.forward(x).shape, generator=g).cuda().bfloat16()
    _, _, dense = _step(m, x, gy, False, extra)
    want = side.forward(dense).clone()
    _, _, deferred = _step(m, x, gy, True, extra)
    assert isinstance(deferred, BNPoolOut)
    torch.testing.assert_close(deferred.dense(), dense, rtol=0, atol=0)
    torch.testing.assert_close(side.forward(deferred), want, rtol=0, atol=0)
    # the pool's deferred gradient, handed to a BN that did not defer: densified, today's path
    pool, bn = m.modules[3], m.modules[1]
    gp = _cl(torch.randn(pool.output.shape, generator=g).cuda().bfloat16())
    pg = pool.updateGradInput(deferred, gp)
    assert isinstance(pg, PoolGrad)
    other = BNOut(deferred.x, deferred.coef, relu=True)  # not the object the BN handed out
    stray = PoolGrad(pg.g, pg.idx, pg.k, pg.s, pg.p, other)
    gi_fused = bn.updateGradInput(m.modules[0].output, pg)
    gi_dense = bn.updateGradInput(m.modules[0].output, stray)
    torch.testing.assert_close(gi_dense.float(), gi_fused.float(), rtol=3e-2, atol=3e-2)
    assert config.get_property("bigdl.fusion.bnpool")
