"""fp32 compute mode: every kernel variant the training compile phase can pin (nn/compiled.py
X3_CANDIDATES for csrc/conv_x3.hip, WGRAD32_CANDIDATES for csrc/conv_wgrad.hip F32) against fp64 torch
on the CPU, under every epilogue / gather mode of the kernels — the compile phase chooses on time alone,
and the other fp32 tests only ever reach the launcher's heuristic for their shape.  A candidate is pinned
the way the compile phase pins it (native_ops._TILE["table"], keyed by the recorded launch geometry) and
the launched instantiation is read back from the kernel name.

  A. every X3 candidate × forward / pointwise / statistics / data gradient (dense, scatter, compact
     strided residual) / BN-backward (recomputed mask, mask bits) / C4 stem / BN prologue;
  B. every fp32 weight-gradient candidate × the four TN × TK tiles on the pointwise and the gather
     branch, split-count edges, dw += scale·… into a non-zero accumulator, deterministic mode, the
     BN prologue;
  C. geometries the direct kernels accept but ResNet never sends (dilation, rectangular filters,
     asymmetric stride / padding, R·S = 64 and 81, tap-less input rows, padding = k − 1);
  D. the asynchronous weight-gradient fork: a backward that ends on the reference op must not have
     written the accumulators first.

Bounds (those of tests/test_fp32_direct.py): relative Frobenius error < 2e-5 for y / gi / gw, < 1e-6 for
the bias gradient, < 1e-5 for epilogue sums.  Reference: F.conv2d + autograd in fp64 on the fp32 inputs
(SpatialConvolution updateOutput / updateGradInput / accGradParameters, DL/nn/SpatialConvolution.scala:
253-505)."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from bigdl.nn.compiled import X3_CANDIDATES, WGRAD32_CANDIDATES

pytestmark = pytest.mark.gpu
dev = "cuda"
cl = torch.channels_last

TOL, TOL_BIAS, TOL_SUMS = 2e-5, 1e-6, 1e-5


# ------------------------------------------------------------------------------------------ helpers
def _cid(c):
    if len(c) == 1:
        return "heur" if c[0] == 0 else f"blocks{-c[0]}"
    bm, bn = c
    return "heur" if bm == 0 else f"{bm}x{bn & 255}" + ("_pix" if bn & 256 else "") + ("_ring2" if bn & 512 else "")


x3_cands = pytest.mark.parametrize("cand", X3_CANDIDATES, ids=_cid)
wg_cands = pytest.mark.parametrize("cand", WGRAD32_CANDIDATES, ids=_cid)
#: part C: the heuristic, the largest tile with the pixels-only wave layout, the smallest tile (2-deep ring)
GEOM_CANDS = ((0, 0), (256, 128 | 256), (128, 64 | 768))

_CUR = ["?"]


@pytest.fixture(autouse=True)
def _name(request):
    _CUR[0] = request.node.name
    yield


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _close(part, what, a, b, tol):
    """Assert rel(a, b) < tol; the figure is printed first (pytest -s / -rP collects them)."""
    e = _rel(a, b)
    print(f"[variants] part={part} test={_CUR[0]} what={what} rel={e:.3e} tol={tol:g}")
    assert e < tol, (what, e)


def _targs(name):
    """Template arguments of a demangled kernel name ("k<a, b>(...)" → ["a", "b"])."""
    head = name.split("(")[0]
    return head.split("<", 1)[1].rstrip(">").split(", ") if "<" in head else []


def _kernels(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _d(t):
    return t.to(dev).contiguous(memory_format=cl) if t.dim() == 4 else t.to(dev)


def _pinned(fn, cand, family, require=True):
    """Run ``fn`` once recording its launch geometries, pin ``cand`` for every recorded ``family`` key
    (as select_kernels does), run it again under the profiler: (result, kernel names).  ``fn`` builds
    its own outputs / accumulators, so the two runs are independent."""
    from bigdl.ops import native_ops as NO
    rec = NO._TILE["record"] = {}
    try:
        fn()
    finally:
        NO._TILE["record"] = None
    torch.cuda.synchronize()
    keys = [k for k in rec if isinstance(k, tuple) and k and k[0] == family]
    assert keys or not require, f"no {family} launch recorded: {list(rec)}"
    table = NO._TILE["table"]
    held = {k: table[k] for k in keys if k in table}   # (a choice an earlier compile phase pinned)
    try:
        for k in keys:
            table[k] = cand
        return _kernels(fn)   # (a candidate the launcher rejects raises RuntimeError: a failure)
    finally:
        for k in keys:
            table.pop(k, None)
        table.update(held)


def _x3_inst(cand):
    """[BM, BN, WM, WN, NS] of the k_conv_x3 instantiation conv_x3.hip's launch_x3 selects for a pinned
    (bm, bn | bits) — None for (0, 0), where the launcher's own heuristic chooses."""
    bm, bn = cand
    if bm == 0:
        return None
    wl, ring2, bn = (bn >> 8) & 1, (bn >> 9) & 1, bn & 0xFF
    if bm == 128 and bn == 64:
        inst = (128, 64, 4, 1, 2)
    elif bm == 128:
        inst = (128, 128, 4 if wl else 2, 1 if wl else 2, 2 if ring2 else 3)
    else:
        inst = (256, bn, 8 if wl else 4, 1 if wl else 2, 3)
    return [str(v) for v in inst]


def _check_x3(names, cand, mode=None, pro=False, launches=None):
    """Every k_conv_x3<BM, BN, WM, WN, MODE, NS, PRO> launched is the pinned instantiation."""
    ts = [_targs(n) for n in names if "k_conv_x3" in n]
    assert ts, names
    inst = _x3_inst(cand)
    for t in ts:
        assert len(t) == 7, t
        if inst is not None:
            assert t[:4] + [t[5]] == inst, (t, inst)
        assert mode is None or t[4] == str(mode), t
        assert t[6] == ("true" if pro else "false"), t
    assert launches is None or len(ts) == launches, names


@functools.lru_cache(maxsize=None)
def _case(N, C, K, H, W, R, S, stride, pad, dil=(1, 1), bias=True, seed=0, need_gi=True):
    """fp32 inputs of one conv and its fp64 forward / gradients (computed once per geometry)."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) * (1.0 / (C * R * S) ** 0.5)
    b = torch.randn(K, generator=g) if bias else None
    xr = x.double().requires_grad_(need_gi)
    wr = w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    yr = F.conv2d(xr, wr, br, stride, pad, dil)
    gy = torch.randn(yr.shape, generator=g)
    ins = [t for t in (xr if need_gi else None, wr, br) if t is not None]
    grads = list(torch.autograd.grad(yr, ins, gy.double()))
    gi = grads.pop(0) if need_gi else None
    gw = grads.pop(0)
    gb = grads.pop(0) if bias else gy.double().sum((0, 2, 3))
    # accumulators to start from: random, of the gradient's magnitude (KRSC physical, like the arena)
    G0 = torch.randn(K, R, S, C, generator=g) * float(gw.std())
    B0 = torch.randn(K, generator=g) * float(gb.std())
    return SimpleNamespace(x=x, w=w, b=b, gy=gy, y=yr.detach(), gi=gi, gw=gw, gb=gb, G0=G0, B0=B0,
                           stride=stride, pad=pad, dil=dil)


def _fwd(c, relu=False, **kw):
    from bigdl.ops import fp32x3 as F3
    xd, wd, bd = _d(c.x), c.w.to(dev), None if c.b is None else c.b.to(dev)
    return lambda: F3.conv_forward(xd, wd, bd, c.stride, c.pad, c.dil, 1, relu, **kw)


def _bwd(c, need_input=True, acc=False, scale=1.0, **kw):
    """``fn`` → (gi, gw, gb) of one F3.conv_backward; ``acc``: into fresh copies of the case's non-zero
    accumulators (else none are passed)."""
    from bigdl.ops import fp32x3 as F3
    xd, wd, gyd = _d(c.x), c.w.to(dev), _d(c.gy)
    G0, B0 = c.G0.to(dev), c.B0.to(dev)
    kw = {k: (_d(v) if isinstance(v, torch.Tensor) and v.dim() == 4 else v) for k, v in kw.items()}

    def fn():
        gw = G0.clone().permute(0, 3, 1, 2) if acc else None
        gb = B0.clone() if acc else None
        gi = F3.conv_backward(gyd, xd, wd, c.stride, c.pad, c.dil, 1, need_input, gw, gb, scale, **kw)
        assert gi is not NotImplemented
        return gi, gw, gb
    return fn


def _check_acc(part, c, gw, gb, scale, gw_ref=None):
    """gw == G0 + scale·ref and gb == B0 + scale·ref_b, the error relative to ‖scale·ref‖."""
    gw_ref = c.gw if gw_ref is None else gw_ref
    _close(part, "gw", gw.double().cpu() - c.G0.double().permute(0, 3, 1, 2), scale * gw_ref, TOL)
    if gb is not None:
        _close(part, "gb", gb.double().cpu() - c.B0.double(), scale * c.gb, TOL_BIAS)


# Part A shapes.  Forward: N = 3 on 13×9 → M = 351 pixels = 128 + 128 + 95 (BM = 128) = 256 + 95 (BM = 256):
# more than one pixel tile and a partial last one for both BM.  K = 200 output channels = 3·64 + 8 = 128 + 72:
# more than one channel tile and a partial last one for both BN.  C = 64, 3×3: 18 k-tiles (1×1: 2).
FWD = dict(N=3, C=64, K=200, H=13, W=9)
# Data gradients swap the roles: the conv's C is the kernel's output side, its K the reduction.
# C = 200 (stride 1) tiles like the forward's K; C = 72 = 64 + 8 (strided) is one partial BN = 128 tile.
DG1 = (3, 200, 64, 13, 9, 3, 3, (1, 1), (1, 1))


# ------------------------------------------------------------------------------ A. X3 candidates
@x3_cands
@pytest.mark.parametrize("K", [200, 32], ids=["K200", "K32"])  # K = 32: fewer channels than either BN
def test_x3_forward_3x3_bias_relu(cand, K):
    c = _case(3, 64, K, 13, 9, 3, 3, (1, 1), (1, 1))
    y, names = _pinned(_fwd(c, relu=True), cand, "x3")
    _check_x3(names, cand, mode=1, launches=1)
    _close("A", "y", y, torch.relu(c.y), TOL)


@x3_cands
@pytest.mark.parametrize("geom", [
    (3, 64, 200, 13, 9, (1, 1)),    # MODE 3, rows read in place (pw_direct); M = 351 as above
    (5, 64, 200, 15, 15, (2, 2)),   # MODE 3 through the strided gather; M = 5·8·8 = 320 = 2·128 + 64 = 256 + 64
], ids=["s1", "s2"])
def test_x3_forward_pointwise(cand, geom):
    N, C, K, H, W, st = geom
    c = _case(N, C, K, H, W, 1, 1, st, (0, 0))
    y, names = _pinned(_fwd(c), cand, "x3")
    _check_x3(names, cand, mode=3, launches=1)
    _close("A", "y", y, c.y, TOL)


# M = 5·13·9 = 585: 5 tiles of BM = 128 (last 73 rows), 3 of BM = 256 (last 73); rep = 2 divides neither
# count and wraps in both (tile tm adds into replica tm % rep)
@x3_cands
@pytest.mark.parametrize("rep", [1, 2])
def test_x3_forward_statistics_epilogue(cand, rep):
    from bigdl.ops import fp32x3 as F3
    c = _case(5, 64, 200, 13, 9, 3, 3, (1, 1), (1, 1), bias=False)
    K = 200
    shift = torch.randn(K, generator=torch.Generator().manual_seed(3)) * 0.1
    xd, wd, sd = _d(c.x), c.w.to(dev), shift.to(dev)
    buf = torch.zeros(2 * rep * K, device=dev)

    def fn():
        buf.zero_()
        r = F3.conv_forward_stats(xd, wd, (1, 1), (1, 1), (1, 1), (buf, rep), sd)
        assert r is not NotImplemented and r[1] is buf and r[2] == rep
        return r[0]
    y, names = _pinned(fn, cand, "x3")
    _check_x3(names, cand, mode=1, launches=1)
    _close("A", "y", y, c.y, TOL)
    yd = y.double().cpu() - shift.double().view(1, K, 1, 1)   # the y the kernel stored
    sums = buf.double().cpu().reshape(2, rep, K).sum(1)
    _close("A", "sum(y-shift)", sums[0], yd.sum((0, 2, 3)), TOL_SUMS)
    _close("A", "sum(y-shift)^2", sums[1], (yd * yd).sum((0, 2, 3)), TOL_SUMS)


@x3_cands
def test_x3_dgrad_stride1_dense_residual(cand):
    c = _case(*DG1)
    res = torch.randn(c.x.shape, generator=torch.Generator().manual_seed(4))
    (gi, _, _), names = _pinned(_bwd(c, residual=res), cand, "x3")
    _check_x3(names, cand, mode=1, launches=1)
    _close("A", "gi", gi, c.gi + res.double(), TOL)


# 3×3 s2 p1 on 15×15: four parity classes of 8×8, 8×7, 7×8, 7×7 pixels per image, N = 5 → 320 / 280 / 280 /
# 245 rows: partial last tiles for both BM; every launch scatters into the 15×15 grid.
# 1×1 s2 p0 on 14×14: one live class (7×7 per image, N = 6 → 294 rows), the other pixels stay zero / = residual.
@x3_cands
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("geom", [(5, 72, 64, 15, 15, 3, 3, (2, 2), (1, 1)), (6, 72, 64, 14, 14, 1, 1, (2, 2), (0, 0))],
                         ids=["3x3s2", "1x1s2"])
def test_x3_dgrad_strided_scatter(cand, geom, res):
    c = _case(*geom)
    r = torch.randn(c.x.shape, generator=torch.Generator().manual_seed(5)) if res else None
    (gi, _, _), names = _pinned(_bwd(c, residual=r), cand, "x3")
    # (3×3 s2: sub-filters of 2×2, 2×1, 1×2 taps on MODE 1 and the 1-tap class on MODE 3)
    _check_x3(names, cand, mode=None if geom[5] == 3 else 3, launches=4 if geom[5] == 3 else 1)
    _close("A", "gi", gi, c.gi + (r.double() if res else 0), TOL)


def _bn_input(shape, seed):
    """A BN input x, scale, shift, mean (fp32) with every |scale·x + shift| ≥ 1e-3 in fp64, so the
    ReLU mask the kernel recomputes in fp32 cannot differ from the fp64 one."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g)
    sc = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    sh, mean = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    t = lambda: sc.double().view(1, C, 1, 1) * x.double() + sh.double().view(1, C, 1, 1)
    x[t().abs() < 1e-3] += 0.01   # |scale| ≥ 0.5: moves the pre-activation by ≥ 5e-3
    assert float(t().abs().min()) >= 1e-3
    return x, sc, sh, mean, t() > 0


def _check_bnbwd(c, g, buf, rep, xb, mean, g_ref):
    C = xb.shape[1]
    _close("A", "g", g, g_ref, TOL)
    gs = g.double().cpu()   # the g the kernel stored
    sums = buf.double().cpu().reshape(2, rep, C).sum(1)
    _close("A", "sum(g)", sums[0], gs.sum((0, 2, 3)), TOL_SUMS)
    _close("A", "sum(g*(x-mean))", sums[1], (gs * (xb.double().cpu() - mean.double().cpu().view(1, C, 1, 1)))
           .sum((0, 2, 3)), TOL_SUMS)


@x3_cands
@pytest.mark.parametrize("geom", [DG1, (5, 72, 64, 15, 15, 3, 3, (2, 2), (1, 1))], ids=["s1", "s2"])
def test_x3_dgrad_bn_backward_recomputed_mask(cand, geom):
    c = _case(*geom)
    C = geom[1]
    xb, sc, sh, mean, mask = _bn_input(c.x.shape, 6)
    rep = 2
    buf = torch.zeros(2 * rep * C, device=dev)
    base = {"x": _d(xb), "mean": mean.to(dev), "scale": sc.to(dev), "shift": sh.to(dev), "sums": (buf, rep)}

    def fn():
        buf.zero_()
        fuse = dict(base)
        gi = _bwd(c, bn_fuse=fuse)()[0]
        assert fuse.get("partial") is buf and fuse.get("G") == rep   # the epilogue took the BN backward
        return gi
    g, names = _pinned(fn, cand, "x3")
    _check_x3(names, cand, mode=1 if geom[7] == (1, 1) else None, launches=1 if geom[7] == (1, 1) else 4)
    _check_bnbwd(c, g, buf, rep, xb, mean, c.gi * mask)


@x3_cands
def test_x3_dgrad_bn_backward_block_tail(cand):
    """Mask bits of the BN + residual + ReLU output (written by the fp32 BN forward) and the shortcut
    gradient as a residual; the mask y > 0 of that output is an input of the op."""
    from bigdl.ops import native_ops as NO
    c = _case(*DG1)
    C = DG1[1]
    g = torch.Generator().manual_seed(7)
    xb = torch.randn(c.x.shape, generator=g)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res, sres = torch.randn(c.x.shape, generator=g), torch.randn(c.x.shape, generator=g)
    xbd = _d(xb)
    y, mean, _ = NO.batchnorm_forward_train(xbd, gam.to(dev), bet.to(dev), torch.zeros(C, device=dev),
                                            torch.ones(C, device=dev), 0.1, 1e-5, relu=True, residual=_d(res))
    rep = 2
    buf = torch.zeros(2 * rep * C, device=dev)

    def fn():
        buf.zero_()
        fuse = {"x": xbd, "mean": mean, "sums": (buf, rep), "mask": y}
        gi = _bwd(c, residual=sres, bn_fuse=fuse)()[0]
        assert fuse.get("partial") is buf and fuse.get("G") == rep
        return gi
    gm, names = _pinned(fn, cand, "x3")
    _check_x3(names, cand, mode=1, launches=1)
    _check_bnbwd(c, gm, buf, rep, xb, mean, (c.gi + sres.double()) * (y.cpu() > 0))


@x3_cands
def test_x3_dgrad_compact_strided_residual(cand):
    """A 1×1 stride-2 shortcut's data gradient kept compact (7×5 of the 13×9 pixels: odd sizes, the last
    row / column of the grid is a residual pixel) and summed by a 3×3 stride-1 data gradient."""
    from bigdl.ops.reference import StridedGrad
    main = _case(3, 72, 64, 13, 9, 3, 3, (1, 1), (1, 1))
    short = _case(3, 72, 64, 13, 9, 1, 1, (2, 2), (0, 0), seed=1)
    f_short = _bwd(short, lazy_strided=True)

    def fn():
        sg = f_short()[0]
        assert isinstance(sg, StridedGrad) and tuple(sg.t.shape) == (3, 72, 7, 5)
        return _bwd(main, residual=sg)()[0]
    gi, names = _pinned(fn, cand, "x3")
    _check_x3(names, cand, launches=2)
    _close("A", "gi", gi, main.gi + short.gi, TOL)


# 7×7 s2 p3 on 3 channels, N = 3 on 30×30 → M = 675 = 5·128 + 35 = 2·256 + 163; K = 136 = 2·64 + 8 = 128 + 8;
# 49 taps = 6 k-tiles of 8 taps + 1 tap
@x3_cands
def test_x3_c4_stem_forward_and_statistics(cand):
    from bigdl.ops import fp32x3 as F3
    from bigdl.utils import config
    c = _case(3, 3, 136, 30, 30, 7, 7, (2, 2), (3, 3), bias=False, need_gi=False)
    K, rep = 136, 4   # 4 divides neither 6 nor 3 M tiles
    config.set_property("bigdl.fp32.stemC4", True)
    try:
        y, names = _pinned(_fwd(c), cand, "x3")
        assert any("k_pad4_f32" in n for n in names), names
        _check_x3(names, cand, mode=2, launches=1)
        _close("A", "y", y, c.y, TOL)
        shift = torch.randn(K, generator=torch.Generator().manual_seed(8)) * 0.1
        xd, wd, sd = _d(c.x), c.w.to(dev), shift.to(dev)
        buf = torch.zeros(2 * rep * K, device=dev)

        def fn():
            buf.zero_()
            r = F3.conv_forward_stats(xd, wd, (2, 2), (3, 3), (1, 1), (buf, rep), sd)
            assert r is not NotImplemented
            return r[0]
        ys, names = _pinned(fn, cand, "x3")
        _check_x3(names, cand, mode=2, launches=1)
        _close("A", "y(stats)", ys, c.y, TOL)
        yd = ys.double().cpu() - shift.double().view(1, K, 1, 1)
        sums = buf.double().cpu().reshape(2, rep, K).sum(1)
        _close("A", "sum(y-shift)", sums[0], yd.sum((0, 2, 3)), TOL_SUMS)
        _close("A", "sum(y-shift)^2", sums[1], (yd * yd).sum((0, 2, 3)), TOL_SUMS)
    finally:
        config.clear_property("bigdl.fp32.stemC4")


@functools.lru_cache(maxsize=None)
def _pro_case(N, C, K, H, W, k, pad):
    """A conv whose input is a deferred BN + ReLU output: x, coef = [scale | shift], and the fp64
    conv(relu(x·scale + shift)) with its weight gradient."""
    g = torch.Generator().manual_seed(40 + k)
    xb = torch.randn(N, C, H, W, generator=g) * 2 + 0.3
    coef = torch.cat([torch.rand(C, generator=g) * 1.5 - 0.25, torch.randn(C, generator=g) * 0.5])
    act = torch.relu(xb.double() * coef[:C].double().view(1, C, 1, 1) + coef[C:].double().view(1, C, 1, 1))
    c = _case(N, C, K, H, W, k, k, (1, 1), (pad, pad), seed=k)
    wr = c.w.double().requires_grad_()
    yr = F.conv2d(act, wr, c.b.double(), 1, pad)
    gw, = torch.autograd.grad(yr, wr, c.gy.double())
    return SimpleNamespace(c=SimpleNamespace(**{**vars(c), "x": xb}), coef=coef, y=yr.detach(), gw=gw)


@x3_cands
@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0)], ids=["3x3", "1x1"])
def test_x3_forward_bn_prologue(cand, k, pad):
    pc = _pro_case(3, 64, 200, 13, 9, k, pad)   # the FWD shape: padded taps must stay 0, not relu(shift)
    y, names = _pinned(_fwd(pc.c, pro=pc.coef.to(dev)), cand, "x3")
    _check_x3(names, cand, mode=1 if k == 3 else 3, pro=True, launches=1)
    _close("A", "y", y, pc.y, TOL)


# --------------------------------------------------------------- B. fp32 weight-gradient candidates
def _wg32_splits(M, K, Kg, target, deterministic=False):
    """blockIdx.y extent of conv_wgrad.hip wgrad_f32_impl for a pinned -target (0: 512 blocks)."""
    cdiv = lambda a, b: -(-a // b)
    tiles = cdiv(K, 64 if K <= 64 else 128) * cdiv(Kg, 64 if Kg <= 64 else 128)
    want, max_by_work = cdiv(-target if target < 0 else 512, tiles), cdiv(M, 512)
    splits = 1 if deterministic else max(1, min(want, max_by_work))
    mps = cdiv(cdiv(M, splits), 64) * 64   # rows per split, rounded up to 64 pixels
    return cdiv(M, mps)


def _check_wg32(names, TN, TK, pw, pro=False):
    """One k_conv_wgrad<TN, TK, 32, …, PW, F32 = true, PRO> launch."""
    ts = [_targs(n) for n in names if "k_conv_wgrad" in n]
    assert len(ts) == 1 and len(ts[0]) == 9, names
    t = ts[0]
    assert t[:3] == [str(TN), str(TK), "32"] and t[6:] == [str(pw).lower(), "true", str(pro).lower()], t


WG_GEOMS = {
    # name: (N, C, K, H, W, R, S, stride, pad), TN, TK, pointwise branch
    # pointwise (1×1 s1 p0) — M = 351: M % 64 = 31, one split for every candidate (⌈351 / 512⌉ = 1)
    "pw_64x64": ((3, 64, 64, 13, 9, 1, 1, (1, 1), (0, 0)), 64, 64, True),
    "pw_64x128": ((3, 136, 40, 13, 9, 1, 1, (1, 1), (0, 0)), 64, 128, True),    # Kg = 136 = 128 + 8, K = 40 < TN
    "pw_128x64": ((3, 40, 200, 13, 9, 1, 1, (1, 1), (0, 0)), 128, 64, True),    # Kg = 40 < TK, K = 200 = 128 + 72
    # M = 8·13·15 = 1560: 4 splits of 448 rows (last 216) for every candidate
    "pw_128x128": ((8, 136, 200, 13, 15, 1, 1, (1, 1), (0, 0)), 128, 128, True),
    # gather branch
    "g_64x64": ((2, 40, 64, 15, 13, 1, 1, (2, 2), (0, 0)), 64, 64, False),      # 1×1 s2: M = 2·8·7 = 112
    "g_64x128": ((1, 8, 40, 7, 7, 3, 3, (1, 1), (1, 1)), 64, 128, False),       # Kg = 72, M = 49 < 64
    "g_128x64": ((3, 64, 72, 13, 9, 1, 1, (2, 2), (0, 0)), 128, 64, False),     # K = 72 < TN, M = 3·7·5 = 105
    "g_128x128": ((8, 8, 200, 13, 15, 3, 3, (1, 1), (1, 1)), 128, 128, False),  # Kg = 72, M = 1560: 4 splits
    # split counts: M = 6·27·27 = 4374 (M % 64 = 22), tiles = 2·18 = 36, max_by_work = ⌈4374 / 512⌉ = 9.
    #   heuristic / -1024 / -2048 / -4096: want ≥ ⌈512 / 36⌉ = 15 → 9 splits of 512 rows, the last 278;
    #   -256: want = ⌈256 / 36⌉ = 8 → 8 splits of ⌈547 / 64⌉·64 = 576 rows, the last 342
    "splits": ((6, 256, 256, 27, 27, 3, 3, (1, 1), (1, 1)), 128, 128, False),
}
WG_SPLITS = {"pw_128x128": {4}, "g_128x128": {4}, "splits": {8, 9}}


@wg_cands
@pytest.mark.parametrize("name", list(WG_GEOMS))
def test_wgrad32_accumulates_scaled_gradient(cand, name):
    geom, TN, TK, pw = WG_GEOMS[name]
    c = _case(*geom, need_gi=False)
    M, K, Kg = c.gy.numel() // geom[2], geom[2], geom[1] * geom[5] * geom[6]
    counts = {_wg32_splits(M, K, Kg, t[0]) for t in WGRAD32_CANDIDATES}
    assert counts == WG_SPLITS.get(name, {1}), counts   # (the case's comment: what the candidates resolve to)
    (gi, gw, gb), names = _pinned(_bwd(c, need_input=False, acc=True, scale=0.5), cand, "wg32")
    assert gi is None
    _check_wg32(names, TN, TK, pw)
    _check_acc("B", c, gw, gb, 0.5)


def test_wgrad32_deterministic_is_one_split():
    """bigdl.deterministic: one block per weight tile (no atomics) — 4 splits otherwise on this shape."""
    from bigdl.utils import config
    geom, TN, TK, pw = WG_GEOMS["g_128x128"]
    c = _case(*geom, need_gi=False)
    fn = _bwd(c, need_input=False, acc=True, scale=0.5)
    config.set_property("bigdl.deterministic", True)
    try:
        (_, gw, gb), names = _kernels(fn)
        (_, gw2, _), _ = _kernels(fn)
    finally:
        config.set_property("bigdl.deterministic", False)
    _check_wg32(names, TN, TK, pw)
    _check_acc("B", c, gw, gb, 0.5)
    assert torch.equal(gw, gw2)   # single-writer reduction: bit-reproducible


@wg_cands
@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0)], ids=["3x3", "1x1"])
def test_wgrad32_bn_prologue(cand, k, pad):
    pc = _pro_case(3, 64, 200, 13, 9, k, pad)
    fn = _bwd(pc.c, need_input=False, acc=True, scale=0.5, pro=pc.coef.to(dev))
    (_, gw, gb), names = _pinned(fn, cand, "wg32")
    _check_wg32(names, 128, 128 if k == 3 else 64, k == 1, pro=True)
    _check_acc("B", pc.c, gw, gb, 0.5, gw_ref=pc.gw)


# ----------------------------------------------------- C. geometries the direct kernels accept
GEOMS = {
    # name: (N, C, K, H, W, R, S, stride, pad, dilation), forward on conv_x3, data gradient on conv_x3
    # (None: whichever family takes it)
    "dilation2": ((2, 32, 64, 11, 9, 3, 3, (1, 1), (2, 2), (2, 2)), True, False),  # C = 32: direct forward
    "1x7": ((2, 32, 64, 9, 13, 1, 7, (1, 1), (0, 3), (1, 1)), True, None),
    "7x1": ((2, 32, 64, 13, 9, 7, 1, (1, 1), (3, 0), (1, 1)), True, None),
    "stride2x1": ((2, 32, 64, 12, 9, 3, 3, (2, 1), (1, 0), (1, 1)), True, None),   # H ≠ W, 6×7 outputs
    "8x8": ((2, 32, 32, 12, 12, 8, 8, (1, 1), (3, 3), (1, 1)), True, True),        # R·S = 64: MODE 1's last
    "9x9": ((2, 32, 32, 12, 12, 9, 9, (1, 1), (4, 4), (1, 1)), False, False),      # R·S = 81: not direct
    # stride 3 > filter 2 on 10×10: input rows / columns 2, 5 get no tap, 8 and 9 lie past the last window
    "s3_2x2": ((2, 32, 64, 10, 10, 2, 2, (3, 3), (0, 0), (1, 1)), True, None),
    "pad_k-1": ((2, 32, 64, 9, 7, 3, 3, (1, 1), (2, 2), (1, 1)), True, True),      # pd = 0 in the dgrad
}


@pytest.mark.parametrize("cand", GEOM_CANDS, ids=_cid)
@pytest.mark.parametrize("name,res", [(n, False) for n in GEOMS] + [("s3_2x2", True)],
                         ids=list(GEOMS) + ["s3_2x2_residual"])
def test_direct_geometry(cand, name, res):
    geom, fwd_x3, dg_x3 = GEOMS[name]
    c = _case(*geom)
    y, names = _pinned(_fwd(c), cand, "x3", require=fwd_x3)
    assert any("k_conv_x3" in n for n in names) == fwd_x3, names
    if fwd_x3:
        _check_x3(names, cand, mode=1, launches=1)
    _close("C", "y", y, c.y, TOL)
    r = torch.randn(c.x.shape, generator=torch.Generator().manual_seed(9)) if res else None
    (gi, gw, gb), names = _pinned(_bwd(c, acc=True, scale=1.0, residual=r), cand, "x3", require=bool(dg_x3))
    if dg_x3 is not None:
        assert any("k_conv_x3" in n for n in names) == dg_x3, names
    if any("k_conv_x3" in n for n in names):
        _check_x3(names, cand)
    # the one-launch fp32 weight gradient takes every one of these
    assert sum("k_conv_wgrad" in n and _targs(n)[7:] == ["true", "false"] for n in names) == 1, names
    _close("C", "gi", gi, c.gi + (r.double() if res else 0), TOL)
    _check_acc("C", c, gw, gb, 1.0)


# ------------------------------------- D. the asynchronous weight-gradient fork accumulates once
ASYNC = {
    # name: (N, C, K, H, W, R, S, stride, pad, dilation), a conv2d_backward fallback is expected
    "1x1_pad1": ((2, 32, 32, 9, 7, 1, 1, (1, 1), (1, 1), (1, 1)), True),    # padding > dilation·(k − 1): no
    "3x3_pad3": ((2, 32, 32, 9, 7, 3, 3, (1, 1), (3, 3), (1, 1)), True),    # native data gradient
    "3x3_dil2": ((2, 32, 32, 9, 7, 3, 3, (1, 1), (2, 2), (2, 2)), False),   # direct dgrad refuses, split takes it
    "K40": ((2, 32, 40, 9, 7, 3, 3, (1, 1), (1, 1), (1, 1)), False),        # K % 32: dgrad on the split path
}


@pytest.mark.parametrize("name", list(ASYNC))
def test_async_wgrad_accumulates_once(name):
    """With the weight gradient forked onto the side stream, every gradient is added exactly once —
    also when the fp32 entry point ends in NotImplemented and the dispatcher runs the reference op
    with the same accumulators (a fork before that decision doubled gw and gb)."""
    from bigdl import ops
    from bigdl.ops import native_ops as NO
    geom, falls_back = ASYNC[name]
    c = _case(*geom)
    xd, wd, gyd = _d(c.x), c.w.to(dev), _d(c.gy)
    gw, gb = c.G0.to(dev).permute(0, 3, 1, 2), c.B0.to(dev)
    ops.reset_fallbacks()
    NO.async_wgrad(True)
    try:
        gi = ops.conv2d_backward(gyd, xd, wd, c.stride, c.pad, c.dil, 1, True, gw, gb, 0.5)
        NO.join_wgrad()
        torch.cuda.synchronize()
    finally:
        NO.async_wgrad(False)
    fb = {k[0] for k in ops.fallback_counts()}
    if not falls_back:
        assert "conv2d_backward" not in fb, ops.fallback_counts()
    _close("D", "gi", gi, c.gi, TOL)
    _check_acc("D", c, gw, gb, 0.5)


def test_async_wgrad_module_accumulates_once():
    """The same through a layer: a 1×1 convolution with padding 1 in fp32 compute mode."""
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.nn import SpatialConvolution
    from bigdl.ops import native_ops as NO
    config.set_property("bigdl.compute.dtype", "fp32")
    try:
        Engine.init(device="cuda:0")
        torch.manual_seed(0)
        m = SpatialConvolution(32, 32, 1, 1, 1, 1, 1, 1)
        w, b = (p.detach().double().clone() for p in m.parameters()[0])
        g = torch.Generator().manual_seed(12)
        x, gy = torch.randn(2, 32, 9, 7, generator=g), torch.randn(2, 32, 11, 9, generator=g)
        m.cuda()
        y = m.forward(x.to(dev))
        m.zeroGradParameters()
        NO.async_wgrad(True)
        try:
            gi = m.backward(x.to(dev), gy.to(dev))
            NO.join_wgrad()
            torch.cuda.synchronize()
        finally:
            NO.async_wgrad(False)
        xr, wr, br = x.double().requires_grad_(), w.reshape(32, 32, 1, 1).requires_grad_(), b.requires_grad_()
        yr = F.conv2d(xr, wr, br, 1, 1)
        yr.backward(gy.double())
        _close("D", "y", y, yr.detach(), TOL)
        _close("D", "gi", gi, xr.grad, TOL)
        _close("D", "gradWeight", m.gradWeight.detach().reshape(32, 32, 1, 1), wr.grad, TOL)
        _close("D", "gradBias", m.gradBias.detach().reshape(-1), br.grad, TOL_BIAS)
    finally:
        config.set_property("bigdl.compute.dtype", "bf16")
        Engine.init(device="cuda:0")
