"""bf16 compute mode (the benchmarked path): every kernel variant the training compile phase can pin
(nn/compiled.py TILE_CANDIDATES for csrc/conv_igemm.hip + csrc/conv_mfma32.hip, WGRAD_CANDIDATES +
WGRAD_EXTRA for csrc/conv_wgrad.hip) against fp64 torch on the CPU, under every epilogue the launchers
give those tiles.  The compile phase chooses on time alone and the other bf16 conv tests reach only the
launcher's heuristic (tests/test_conv_x8.py: the four x8 tiles, forward only, at 2e-2).  A candidate is
pinned the way the compile phase pins it (native_ops._TILE["table"], keyed by the recorded launch
geometry) and the launched instantiation is read back from the kernel name.

  A. every TILE_CANDIDATES entry × forward epilogues (_conv_fwd_impl): bias + ReLU, dense residual,
     strided output slice (zero-copy concat), BN statistics as partial rows / [2K + 1] atomic / replicas;
  B. every TILE_CANDIDATES entry × backward-data (_dgrad_s1, the lazy 1×1 strided launch): plain, dense
     and compact strided residual, the BN-backward epilogue with the recomputed mask (three sums
     layouts), the block tail as mask tensor, mask bits, and bits + strided residual;
  C. every WGRAD_CANDIDATES + WGRAD_EXTRA entry × the pointwise, gather and C4-stem branches of
     wgrad_launch, split-count edges, dw += scale·… into a non-zero accumulator, deterministic mode;
  D. re-timing (_TILE["retiming"]) must not add into the caller's live BN sums.

Reference: inputs are generated in fp32 and rounded to bf16 once; F.conv2d + autograd in fp64 on those
values (SpatialConvolution updateOutput / updateGradInput / accGradParameters, DL/nn/
SpatialConvolution.scala:253-505), cached per geometry.

Bounds (none taken from the code under test):
  y / gi per element   |got − ref| ≤ 2⁻⁸·|ref| + 2e-5·rms(ref); 2⁻⁸ = bf16 unit roundoff, the absolute
                       term covers fp32 accumulation (a torch fp32 CPU conv of the part-A shapes is within
                       5–9e-7 of fp64 at rms ≈ 1).  Masked elements are exactly 0.
  y / gi Frobenius     rel(got, ref) ≤ 1.05 × rel(bf16(ref), ref) (the floor is computed per comparison;
                       1.655–1.669e-3 on the part-A shapes).
  Σ(y−s)               |got − ref| ≤ 2⁻⁶·√(Σ_m y²) per channel (≈ 8σ of the roundings' random walk;
                       conv_store_pass sums either the fp32 accumulators or the stored bf16 values)
  Σ(y−s)²              |got − ref| ≤ 2⁻⁵·√(Σ_m (y−s)²·y²)
  Σg', Σg'·(x−μ)       |got − ref| ≤ 2⁻⁶·√(Σ_m g'²), 2⁻⁶·√(Σ_m (g'·(x−μ))²)
  gw (fp32)            relative Frobenius error of gw − G0 vs scale·ref < 2e-5, gb < 1e-6 (the bounds of
                       tests/test_fp32_direct.py; bf16 products are exact in fp32).
The sums are compared with the fp64 reference, never with the kernel's own stored output.  The
bf16-rounded reference alone (rounded outputs summed in fp64), maximum over the channels, as a fraction of
each bound on the shapes used here:
  Σ(y−s)   0.30 (S3) 0.38 (S1) 0.32 (F1s2) 0.37 (S72), with bias 0.32 / 0.35 / 0.35 / 0.30;
  Σ(y−s)²  0.30 / 0.37 / 0.37 / 0.33, with bias 0.33 / 0.34 / 0.33 / 0.32;
  Σg'      0.30 (D1) 0.30 (D1x1) 0.27 (D72) recomputed mask, 0.33 / 0.33 / 0.44 block tail (random mask);
  Σg'·(x−μ) 0.37 / 0.31 / 0.29 recomputed mask, 0.31 / 0.42 / 0.34 block tail
— all below one half, so the coefficients stand as stated.

Both kernel families park the fp32 accumulator (+ bias) as bf16 in LDS before the shared store pass adds a
residual (conv_igemm.hip "park ... as bf16", conv_mfma32.hip "park the tile as bf16", conv_params.h
conv_store_pass: unpack8(rd_chunk) + residual, f2bf), so y = bf16(bf16(conv + bias) + res) by design.  The
reference models that: expected = bf16(ref_conv) + res.  Where ref_conv lies within the fp32-accumulation
allowance (2e-5·rms) of a bf16 rounding boundary, either neighbour is a legitimate intermediate, and an
element passes if it meets the per-element bound against any of the three candidates bf16(ref_conv),
bf16(ref_conv ± 2e-5·rms) (≈ 3.5 % of the elements have more than one; a wrong row has none that fits).

Instantiations launched (asserted from the kernel names), by epilogue class:

  family / tiles              MODE  A: bias+ReLU  residual  out=  statistics  B: plain/res  strided res  BN-bwd  tail
  k_conv_fwd, 6 (BN×BK×BM):   0     G72 C8 (G96)  G72       G72   S72         D72           D72          D72     D72
    64/128 × 32/64 × 128,     1     F3 F3s2 …     F3        F3    S3          D1 D1p0       D1           D1      D1
    64/128 × 64 × 256         3     F1 F1s2 tiny  F1        F1    S1 F1s2     D1x1          D1x1 + lazy  D1x1    D1x1
  k_conv_x8, 4 (BM×BN):       1     F3 F3s2 K32 … F3        F3    S3          D1 D1p0       D1           D1      D1
    128×128 256×64/128/256    3     F1 F1s2 tiny  F1        F1    S1 F1s2     D1x1          D1x1 + lazy  D1x1    D1x1
  (x8 candidates on C % 64 ≠ 0 — G72, G96, C8, S72, D72 — assert the documented fall-back to the
  heuristic k_conv_fwd instantiation.)
  k_conv_wgrad, TN×TK × depth 32/64: PW1 (64×64, 64×128, 128×64, 128×128), gather (128×128 3×3 s1 / s2,
  128×64 1×1 s2), C4 (128×128) — every branch at both depths through the (·, 32) and (·, 64) candidates.
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from bigdl.nn.compiled import TILE_CANDIDATES, WGRAD_CANDIDATES, WGRAD_EXTRA

pytestmark = pytest.mark.gpu
dev = "cuda"
cl = torch.channels_last

U = 2.0 ** -8          # bf16 unit roundoff
ABS = 2e-5             # fp32-accumulation allowance, × rms(ref)
FROB = 1.05            # × the bf16 rounding floor of the reference
C_SUM, C_SQ = 2.0 ** -6, 2.0 ** -5
TOL_GW, TOL_GB = 2e-5, 1e-6

WG_ALL = tuple(WGRAD_CANDIDATES) + tuple(WGRAD_EXTRA)
assert len(TILE_CANDIDATES) == 11 and len(WG_ALL) == 13


# ------------------------------------------------------------------------------------------ helpers
def _cid(c):
    if len(c) == 3:
        bn, bk, bm = c
        return "heur" if c == (0, 0, 0) else (f"x8_{bm}x{bn}" if bk == 1 else f"bn{bn}_bk{bk}_bm{bm}")
    return f"blocks{c[0]}_bp{c[1]}"


tile_cands = pytest.mark.parametrize("cand", TILE_CANDIDATES, ids=_cid)
wg_cands = pytest.mark.parametrize("cand", WG_ALL, ids=_cid)

_CUR = ["?"]


@pytest.fixture(autouse=True)
def _name(request):
    _CUR[0] = request.node.name
    yield


def _report(part, what, val, tol, strict=False):
    """One figure, printed before it is asserted (pytest -s / -rP collects the lines)."""
    print(f"[variants] part={part} test={_CUR[0]} what={what} rel={val:.3e} tol={tol:g}")
    assert (val < tol) if strict else (val <= tol), (what, val, tol)


def _bf(t):
    """Round to bf16 once; returned as fp64 (exact)."""
    return t.float().bfloat16().double()


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _close(part, what, got, ref, alts=(), zero=None):
    """``got`` (a bf16 kernel output) against the fp64 ``ref``: the per-element bound (against ``ref`` or
    any of ``alts``, see the module docstring), the Frobenius bound against ``ref``, and exact zeros where
    ``zero`` is set."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    rms = float(ref.pow(2).mean().sqrt())
    q = (got - ref).abs() / (U * ref.abs() + ABS * rms)
    for r in alts:
        q = torch.minimum(q, (got - r).abs() / (U * r.abs() + ABS * rms))
    _report(part, what + ":elem", float(q.max()), 1.0)
    _report(part, what + ":frob", _rel(got, ref), FROB * _rel(_bf(ref), ref))
    if zero is not None:
        assert int((got[zero] != 0).sum()) == 0, what


def _close_sums(part, what, got, ref, unit_sq, coef):
    """Per channel |got − ref| ≤ coef·√unit_sq."""
    r = (got.double().cpu() - ref).abs() / unit_sq.sqrt().clamp_min(1e-300)
    _report(part, what, float(r.max()), coef)


def _inter(v):
    """The legitimate bf16 intermediates of an fp64 value the kernels round before a residual add: the
    rounded value first, then its neighbours where v is within the accumulation allowance of a tie."""
    a = ABS * float(v.pow(2).mean().sqrt())
    return [_bf(v), _bf(v - a), _bf(v + a)]


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
    """bf16 on the device, channels-last for activations / filters."""
    t = t.to(dev).bfloat16()
    return t.contiguous(memory_format=cl) if t.dim() == 4 else t


def _family(k):
    return "wg" if (isinstance(k, tuple) and k and k[0] == "wg") else \
        ("conv" if (isinstance(k, tuple) and k and isinstance(k[0], int)) else None)


def _pinned(fn, cand, family="conv"):
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
    keys = [k for k in rec if _family(k) == family]
    assert keys, f"no {family} launch recorded: {list(rec)}"
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


def _igemm_inst(cand, C, K, R, S, pad):
    """The instantiation conv_fwd_launch (conv_igemm.hip) selects for a pinned (BN, BK, BM) on a conv with
    C reduction channels (C % 8 == 0) and K output channels: ("x8", BM, BN, MODE) for k_conv_x8<BM, BN, …,
    MODE, …> or ("fwd", BN, MODE, BM, BK) for k_conv_fwd<BN, MODE, BM, BK, …>.  An x8 candidate (BK = 1) on
    a shape conv_x8_ok refuses (C % 64 ≠ 0) takes the heuristic 16×16×32 tile, as (0, 0, 0) does."""
    bn, bk, bm = cand
    Kg = R * S * C
    pw = R == 1 and S == 1 and tuple(pad) == (0, 0)
    if bk == 1:
        if C % 64 == 0 and (pw or R * S <= 64):
            return ("x8", bm, bn, 3 if pw else 1)
        bn = bk = bm = 0
    BN = bn or (64 if K <= 64 else 128)
    BK = bk or (32 if Kg <= 512 else 64)
    if not bk and BK == 64 and C % 64 != 0 and C % 32 == 0:
        BK = 32
    BM = bm or 128
    fast = C % BK == 0 and R * S <= 64
    return ("fwd", BN, (3 if pw else 1) if fast else 0, BM, BK)


def _launched(names):
    """The implicit-GEMM conv launches of a profile, in _igemm_inst's form; the opt-in patch kernel must
    not have intercepted any."""
    assert not any("k_conv_patch" in n for n in names), names
    out = []
    for n in names:
        if "k_conv_fwd<" in n:
            t = _targs(n)
            assert len(t) == 6 and t[4:] == ["false", "false"], n
            out.append(("fwd", int(t[0]), int(t[1]), int(t[2]), int(t[3])))
        elif "k_conv_x8<" in n:
            t = _targs(n)
            assert len(t) == 6, n
            out.append(("x8", int(t[0]), int(t[1]), int(t[4])))
    return out


def _check_conv(names, cand, *geoms):
    """Exactly the expected instantiations ran, one per (C, K, R, S, pad) kernel-side geometry, in order."""
    want = [_igemm_inst(cand, *g) for g in geoms]
    got = _launched(names)
    assert got == want, (got, want, names)


@functools.lru_cache(maxsize=None)
def _case(N, C, K, H, W, R, S, stride, pad, seed=0):
    """bf16-valued inputs of one conv and its fp64 forward (without bias) / gradients, once per geometry."""
    g = torch.Generator().manual_seed(100 + seed)
    x = _bf(torch.randn(N, C, H, W, generator=g)).float()
    w = _bf(torch.randn(K, C, R, S, generator=g) * (1.0 / (C * R * S) ** 0.5)).float()
    b = torch.randn(K, generator=g)                       # the launchers take an fp32 bias
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr, wr, None, stride, pad)
    gy = _bf(torch.randn(yr.shape, generator=g)).float()
    gi, gw = torch.autograd.grad(yr, (xr, wr), gy.double())
    gb = gy.double().sum((0, 2, 3))
    # accumulators to start from: random, of the gradient's magnitude (KRSC physical, like the arena)
    G0 = torch.randn(K, R, S, C, generator=g) * float(gw.std())
    B0 = torch.randn(K, generator=g) * float(gb.std())
    return SimpleNamespace(x=x, w=w, b=b, gy=gy, y=yr.detach(), yb=yr.detach() + b.double().view(1, K, 1, 1),
                           gi=gi, gw=gw, gb=gb, G0=G0, B0=B0, stride=stride, pad=pad, geom=(N, C, K, H, W, R, S),
                           M=yr.numel() // K)


def _kgeom(c):
    """Kernel-side geometry of the forward: (C padded to 8, K, R, S, pad)."""
    N, C, K, H, W, R, S = c.geom
    return ((C + 7) // 8 * 8, K, R, S, c.pad)


def _dgeom(c):
    """Kernel-side geometry of the stride-1 data gradient: reduction over the conv's K, output the conv's C,
    padding k − 1 − pad."""
    N, C, K, H, W, R, S = c.geom
    return (K, C, R, S, (R - 1 - c.pad[0], S - 1 - c.pad[1]))


s1, s2, p0, p1 = (1, 1), (2, 2), (0, 0), (1, 1)

# Part A shapes: (N, C, K, H, W, R, S, stride, pad).
FWD = {
    # M = 3·13·9 = 351 = 2·128 + 95 = 256 + 95: three 128-row statistics rows, the last BM = 256 tile's second
    # half wholly past M.  K = 264 = 4·64 + 8 = 2·128 + 8 = 256 + 8: a full and an 8-channel partial tile
    # for every BN (store pass: n0 + BN ≤ K vs the tail).  Kg = 576 = 9 k-tiles of 64 (18 of 32).
    "F3": (3, 64, 264, 13, 9, 3, 3, s1, p1),
    # Kg = 64: ONE k-tile of 64 (two of 32) — shorter than any ring / prefetch depth; MODE 3, rows in place
    "F1": (3, 64, 264, 13, 9, 1, 1, s1, p0),
    "F1c128": (3, 128, 264, 13, 9, 1, 1, s1, p0),   # Kg = 128: two k-tiles of 64
    # M = 5·8·8 = 320 = 2·128 + 64 = 256 + 64; MODE 3 through the strided gather / 3×3 stride 2
    "F1s2": (5, 64, 264, 15, 15, 1, 1, s2, p0),
    "F3s2": (5, 64, 264, 15, 15, 3, 3, s2, p1),
    "G72": (3, 72, 264, 13, 9, 3, 3, s1, p1),       # C % 32 ≠ 0: MODE 0 under both BK; x8 falls back
    "G96": (3, 96, 264, 13, 9, 3, 3, s1, p1),       # tap-uniform at BK 32, generic at BK 64; x8 falls back
    "K32": (3, 64, 32, 13, 9, 3, 3, s1, p1),        # K smaller than every BN
    "K100": (3, 64, 100, 13, 9, 3, 3, s1, p1),      # K % 8 ≠ 0: the per-element store tail (plain forward only)
    "tiny": (1, 64, 264, 7, 7, 1, 1, s1, p0),       # M = 49: less than one tile
    "C8": (3, 8, 264, 13, 9, 1, 1, s1, p0),         # Kg = 8 < BK: MODE 0 pointwise; x8 falls back
    # statistics: M = 5·13·9 = 585 = 4·128 + 73 = 2·256 + 73: five statistics rows; rep = 2 divides neither the
    # BM = 128 (5) nor the BM = 256 (3) tile count and wraps in both (row group g adds into replica g % rep)
    "S3": (5, 64, 264, 13, 9, 3, 3, s1, p1),
    "S1": (5, 64, 264, 13, 9, 1, 1, s1, p0),
    "S72": (5, 72, 264, 13, 9, 3, 3, s1, p1),       # MODE 0
}
ALL_SHAPES = ["F3", "F1", "F1c128", "F1s2", "F3s2", "G72", "G96", "K32", "K100", "tiny", "C8"]
EPI_SHAPES = ["F3", "F1", "G72"]                    # MODE 1 / 3 / 0 (x8: 1 / 3 / fall-back)
STAT_SHAPES = ["S3", "S1", "F1s2", "S72"]


def _fwd_args(c):
    return _d(c.x), _d(c.w), c.b.to(dev)


# -------------------------------------------------------------- A. tile candidates × forward epilogues
@tile_cands
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_fwd_bias_relu(cand, shape):
    from bigdl.ops import native_ops as NO
    c = _case(*FWD[shape])
    xd, wd, bd = _fwd_args(c)
    y, names = _pinned(lambda: NO.conv2d_forward(xd, wd, bd, c.stride, c.pad, (1, 1), 1, True), cand)
    assert y is not NotImplemented
    _check_conv(names, cand, _kgeom(c))
    _close("A", "y", y, torch.relu(c.yb))


@tile_cands
@pytest.mark.parametrize("relu", [False, True], ids=["sum", "sum_relu"])
@pytest.mark.parametrize("shape", EPI_SHAPES)
def test_fwd_dense_residual(cand, shape, relu):
    from bigdl.ops import native_ops as NO
    c = _case(*FWD[shape])
    xd, wd, bd = _fwd_args(c)
    res = _bf(torch.randn(c.y.shape, generator=torch.Generator().manual_seed(4)))
    rd = _d(res)
    y, names = _pinned(lambda: NO.conv2d_forward(xd, wd, bd, c.stride, c.pad, (1, 1), 1, relu, None, rd), cand)
    assert y is not NotImplemented
    _check_conv(names, cand, _kgeom(c))
    act = torch.relu if relu else (lambda t: t)
    refs = [act(v + res) for v in _inter(c.yb)]   # bf16(conv + bias), then + res (module docstring)
    _close("A", "y", y, refs[0], refs[1:])


@tile_cands
@pytest.mark.parametrize("shape", EPI_SHAPES)
def test_fwd_strided_output_slice(cand, shape):
    """out = big[:, 40:304] of a 304-channel channels-last tensor (ldy = 304 ≠ K = 264): the slice holds the
    conv, every channel outside it is bit-unchanged."""
    from bigdl.ops import native_ops as NO
    c = _case(*FWD[shape])
    N, C, K, H, W, R, S = c.geom
    xd, wd, bd = _fwd_args(c)
    P, Q = c.y.shape[2:]
    SENT = -1232.0   # exact in bf16 (7 significant bits)

    def fn():
        big = torch.full((N, 304, P, Q), SENT, dtype=torch.bfloat16, device=dev).contiguous(memory_format=cl)
        r = NO.conv2d_forward(xd, wd, bd, c.stride, c.pad, (1, 1), 1, True, big[:, 40:304])
        assert r is not NotImplemented and r.data_ptr() == big[:, 40:304].data_ptr()
        return big
    big, names = _pinned(fn, cand)
    _check_conv(names, cand, _kgeom(c))
    assert bool((big[:, :40] == SENT).all()), "channels before the slice were written"
    _close("A", "y", big[:, 40:304], torch.relu(c.yb))


@tile_cands
@pytest.mark.parametrize("layout", ["rows", "atomic", "rep1", "rep2"])
@pytest.mark.parametrize("shape", STAT_SHAPES)
def test_fwd_statistics(cand, shape, layout):
    """Σ(y − shift), Σ(y − shift)² per channel in the three layouts the launcher accepts.  "rows" runs with a
    bias (the store pass sums the stored bf16 values in every tile), the atomic layouts without (BM = 128
    16×16×32 tiles sum the fp32 accumulators)."""
    from bigdl.ops import native_ops as NO
    c = _case(*FWD[shape])
    K, M = c.geom[2], c.M
    xd, wd, bd = _fwd_args(c)
    bias = layout == "rows"
    shift = torch.randn(K, generator=torch.Generator().manual_seed(3)) * 0.1
    sd = shift.to(dev)
    rep = {"rows": 0, "atomic": 1, "rep1": 1, "rep2": 2}[layout]
    buf = None if layout == "rows" else torch.zeros(2 * K + 1 if layout == "atomic" else 2 * rep * K, device=dev)
    sums_arg = None if layout == "rows" else (buf if layout == "atomic" else (buf, rep))
    G_rows = -(-M // 128)

    def fn():
        if buf is not None:
            buf.zero_()
        r = NO.conv2d_forward_stats(xd, wd, bd if bias else None, c.stride, c.pad, shift=sd, sums=sums_arg)
        assert r is not NotImplemented
        return r
    (y, part, G), names = _pinned(fn, cand)
    _check_conv(names, cand, _kgeom(c))
    yref = c.yb if bias else c.y
    _close("A", "y", y, yref)
    if layout == "rows":
        assert G == G_rows and part.numel() == 2 * G * K
        sums = part.double().cpu().view(2, G, K).sum(1)
    elif layout == "atomic":
        assert part is buf and G == 0
        assert float(buf[2 * K]) == 0.0   # the consumer's ticket word is not the conv's to write
        sums = buf[:2 * K].double().cpu().view(2, K)
    else:
        assert part is buf and G == rep
        sums = buf.double().cpu().view(2, rep, K).sum(1)
    dd = yref - shift.double().view(1, K, 1, 1)
    _close_sums("A", "sum(y-shift)", sums[0], dd.sum((0, 2, 3)), (yref * yref).sum((0, 2, 3)), C_SUM)
    _close_sums("A", "sum(y-shift)^2", sums[1], (dd * dd).sum((0, 2, 3)), (dd * dd * yref * yref).sum((0, 2, 3)), C_SQ)


# ----------------------------------------------------------- B. tile candidates × backward-data
# The data gradient is a forward conv of gy with the roles swapped: the conv's C = 264 is the kernel's output
# side (tiles like K above), its K the reduction.  N = 3 on 13×9: M = 351 as F3.
DGR = {
    "D1": (3, 264, 64, 13, 9, 3, 3, s1, p1),      # reduction 64·9 = 576: MODE 1 (x8 MODE 1)
    "D1p0": (3, 264, 64, 13, 9, 3, 3, s1, p0),    # gy is 11×7, dgrad padding k − 1 = 2
    "D1x1": (3, 264, 128, 13, 9, 1, 1, s1, p0),   # reduction 128: MODE 3, two k-tiles of 64
    "D72": (3, 264, 72, 13, 9, 3, 3, s1, p1),     # reduction channels 72: MODE 0; x8 falls back
}
DG_EPI = ["D1", "D1x1", "D72"]
# the 1×1 stride-2 shortcut whose gradient stays compact: 7×5 of the 13×9 pixels (odd sizes: the last row and
# column of the grid are residual pixels); its lazy launch is a pointwise conv with M = 105 < one tile
SHORT = (3, 264, 64, 13, 9, 1, 1, s2, p0)


def _bwd(c, **kw):
    """``fn`` → the input gradient of one bf16 NO.conv2d_backward (no weight gradient)."""
    from bigdl.ops import native_ops as NO
    xd, wd, gyd = _d(c.x), _d(c.w), _d(c.gy)

    def fn(**more):
        gi = NO.conv2d_backward(gyd, xd, wd, c.stride, c.pad, (1, 1), 1, True, None, None, 1.0, **kw, **more)
        assert gi is not NotImplemented
        return gi
    return fn


def _res_like(c, seed):
    """A bf16-valued residual gradient of gi's magnitude."""
    return _bf(torch.randn(c.x.shape, generator=torch.Generator().manual_seed(seed)) * float(c.gi.std()))


@tile_cands
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", list(DGR))
def test_dgrad_stride1(cand, shape, res):
    c = _case(*DGR[shape])
    r = _res_like(c, 5) if res else None
    gi, names = _pinned(_bwd(c, residual=None if r is None else _d(r)), cand)
    _check_conv(names, cand, _dgeom(c))
    if res:
        refs = [v + r for v in _inter(c.gi)]
        _close("B", "gi", gi, refs[0], refs[1:])
    else:
        _close("B", "gi", gi, c.gi)


def _short_geom():
    N, C, K, H, W, R, S = SHORT[:7]
    return (K, C, 1, 1, (0, 0))


def _strided(t_full, sg):
    """The dense fp64 image of a StridedGrad's compact tensor."""
    out = torch.zeros(t_full.shape, dtype=torch.float64)
    out[:, :, ::sg.stride[0], ::sg.stride[1]] = sg.t.double().cpu()
    return out


@tile_cands
@pytest.mark.parametrize("shape", DG_EPI)
def test_dgrad_compact_strided_residual(cand, shape):
    """lazy_strided: the shortcut's gradient as a StridedGrad (checked against fp64 on its own), then summed by
    the main conv's data gradient as a strided residual ("conv_dgrad_rs")."""
    from bigdl.ops.reference import StridedGrad
    main, short = _case(*DGR[shape]), _case(*SHORT, seed=1)
    f_short, f_main = _bwd(short, lazy_strided=True), _bwd(main)

    def fn():
        sg = f_short()
        assert isinstance(sg, StridedGrad) and tuple(sg.t.shape) == (3, 264, 7, 5)
        return sg, f_main(residual=sg)
    (sg, gi), names = _pinned(fn, cand)
    _check_conv(names, cand, _short_geom(), _dgeom(main))
    _close("B", "gi(lazy_1x1s2)", sg.t, short.gi[:, :, ::2, ::2])
    assert float(short.gi[:, :, 1::2].abs().max()) == 0.0   # (off-grid pixels of the shortcut carry no gradient)
    r = _strided(main.gi, sg)   # the residual the main launch was given
    refs = [v + r for v in _inter(main.gi)]
    _close("B", "gi", gi, refs[0], refs[1:])


def _bn_input(shape, seed):
    """A bf16-valued BN input x and fp32 scale, shift, mean with every |scale·x + shift| ≥ 1e-3 in fp64 (x is
    rounded BEFORE that is enforced and re-checked after the nudge), so the ReLU mask the kernel recomputes in
    fp32 cannot differ from the fp64 one."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = _bf(torch.randn(shape, generator=g)).float()
    sc = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    sh, mean = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    t = lambda: sc.double().view(1, C, 1, 1) * x.double() + sh.double().view(1, C, 1, 1)
    bad = t().abs() < 1e-3
    # |scale| ≥ 0.5 and a move of ≥ 0.6·nudge after rounding (nudge ≥ 2 ulp): the pre-activation moves ≥ 3e-3
    x[bad] = _bf(x[bad] + torch.clamp(x[bad].abs() * 2.0 ** -6, min=0.01)).float()
    assert float(t().abs().min()) >= 1e-3 and torch.equal(_bf(x).float(), x)
    return x, sc, sh, mean, t() > 0


def _check_bn_sums(sums, g_ref, xb, mean):
    """Σg' and Σg'·(x − μ) per channel against fp64."""
    C = xb.shape[1]
    xm = xb.double() - mean.double().view(1, C, 1, 1)
    _close_sums("B", "sum(g)", sums[0], g_ref.sum((0, 2, 3)), (g_ref * g_ref).sum((0, 2, 3)), C_SUM)
    t = g_ref * xm
    _close_sums("B", "sum(g*(x-mean))", sums[1], t.sum((0, 2, 3)), (t * t).sum((0, 2, 3)), C_SUM)


def _bn_sums_arg(layout, C):
    """(sums argument of bn_fuse, buffer, expected G, reader → [2][C] fp64)."""
    if layout == "rows":
        return None, None, None
    rep = 2
    buf = torch.zeros(2 * C + 1 if layout == "atomic" else 2 * rep * C, device=dev)
    return (buf if layout == "atomic" else (buf, rep)), buf, (0 if layout == "atomic" else rep)


def _read_bn_sums(layout, fuse, buf, C, M):
    if layout == "rows":
        G = -(-M // 128)
        assert fuse.get("G") == G and fuse["partial"].numel() == 2 * G * C   # the epilogue took the BN backward
        return fuse["partial"].double().cpu().view(2, G, C).sum(1)
    assert fuse.get("partial") is buf
    if layout == "atomic":
        assert fuse.get("G") == 0 and float(buf[2 * C]) == 0.0
        return buf[:2 * C].double().cpu().view(2, C)
    assert fuse.get("G") == 2
    return buf.double().cpu().view(2, 2, C).sum(1)


@tile_cands
@pytest.mark.parametrize("layout", ["rows", "atomic", "replicas"])
@pytest.mark.parametrize("shape", DG_EPI)
def test_dgrad_bn_backward_recomputed_mask(cand, shape, layout):
    """conv → BN + ReLU → this conv: g' = gi·[scale·x + shift > 0] and the BN-backward sums, for the partial
    rows (bigdl_conv_fwd_full), the [2C + 1] atomic buffer and replicas (bigdl_conv_fwd_bnbwd)."""
    c = _case(*DGR[shape])
    C, M = c.geom[1], c.x.numel() // c.geom[1]
    xb, sc, sh, mean, mask = _bn_input(c.x.shape, 6)
    sums_arg, buf, _ = _bn_sums_arg(layout, C)
    base = {"x": _d(xb), "mean": mean.to(dev), "scale": sc.to(dev), "shift": sh.to(dev)}
    if sums_arg is not None:
        base["sums"] = sums_arg
    f = _bwd(c)
    last = {}

    def fn():
        if buf is not None:
            buf.zero_()
        fuse = dict(base)
        gi = f(bn_fuse=fuse)
        last["fuse"] = fuse
        return gi
    g, names = _pinned(fn, cand)
    _check_conv(names, cand, _dgeom(c))
    g_ref = c.gi * mask
    _close("B", "g", g, g_ref, zero=~mask)
    _check_bn_sums(_read_bn_sums(layout, last["fuse"], buf, C, M), g_ref, xb, mean)


@functools.lru_cache(maxsize=None)
def _tail(shape):
    """Block tail of ``shape``'s input: y = relu(BN(x) + res) from the bf16 BN forward with its mask bits; the
    mask y > 0 of that output (and the bits, asserted equal to it) are INPUTS of the op under test."""
    from bigdl.ops import native_ops as NO
    c = _case(*DGR[shape])
    N, C, K, H, W, R, S = c.geom
    g = torch.Generator().manual_seed(7)
    xb = _bf(torch.randn(c.x.shape, generator=g)).float()
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res = _bf(torch.randn(c.x.shape, generator=g)).float()
    xbd = _d(xb)
    bits = torch.zeros(N * H * W * C // 8, dtype=torch.uint8, device=dev)
    y, mean, _ = NO.batchnorm_forward_train(xbd, gam.to(dev), bet.to(dev), torch.zeros(C, device=dev),
                                            torch.ones(C, device=dev), 0.1, 1e-5, relu=True, residual=_d(res),
                                            bits_out=bits)
    torch.cuda.synchronize()
    mask = y.float().cpu() > 0
    # bit e of byte [m][n / 8] is channel n + e of pixel m (NHWC)
    dec = ((bits.cpu().view(N * H * W, C // 8, 1).int() >> torch.arange(8).view(1, 1, 8)) & 1).bool()
    assert torch.equal(dec.view(N, H, W, C).permute(0, 3, 1, 2), mask), "BN forward: mask bits ≠ [y > 0]"
    return SimpleNamespace(xb=xb, xbd=xbd, y=y, bits=bits, mean=mean, mask=mask)


@tile_cands
@pytest.mark.parametrize("src", ["mask", "bits", "bits_strided"])
@pytest.mark.parametrize("shape", DG_EPI)
def test_dgrad_bn_backward_block_tail(cand, shape, src):
    """g' = (gi + shortcut gradient)·[block output > 0] with the BN-backward partial rows: the mask as the bf16
    block output (bigdl_conv_fwd_full), as the forward's mask bits (bigdl_conv_fwd_full2), and bits together
    with the compact strided shortcut gradient."""
    from bigdl.ops.reference import StridedGrad
    c, t = _case(*DGR[shape]), _tail(shape)
    C, M = c.geom[1], c.x.numel() // c.geom[1]
    base = {"x": t.xbd, "mean": t.mean, "mask": t.y}
    if src != "mask":
        base["bits"] = t.bits
    f = _bwd(c)
    last = {}
    if src == "bits_strided":
        short = _case(*SHORT, seed=1)
        f_short = _bwd(short, lazy_strided=True)
        geoms = (_short_geom(), _dgeom(c))
    else:
        sres = _res_like(c, 8)
        srd = _d(sres)
        geoms = (_dgeom(c),)

    def fn():
        r = f_short() if src == "bits_strided" else srd
        fuse = dict(base)
        gi = f(residual=r, bn_fuse=fuse)
        last["fuse"], last["res"] = fuse, r
        return gi
    g, names = _pinned(fn, cand)
    _check_conv(names, cand, *geoms)
    if src == "bits_strided":
        assert isinstance(last["res"], StridedGrad)
        sres = _strided(c.gi, last["res"])
    m = t.mask.double()
    refs = [(v + sres) * m for v in _inter(c.gi)]   # bf16(gi), + residual, mask (conv_store_pass)
    _close("B", "g", g, refs[0], refs[1:], zero=~t.mask)
    _check_bn_sums(_read_bn_sums("rows", last["fuse"], None, C, M), refs[0], t.xb, t.mean.cpu())


def test_tile_coverage_of_parts_a_and_b():
    """The module docstring's table, from the parametrisation itself: in every epilogue class each of the six
    k_conv_fwd tiles is launched under MODE 0, 1 and 3 and each of the four k_conv_x8 tiles under MODE 1 and 3
    (the per-test name assertions make _igemm_inst the launched truth), so thinning a shape list cannot
    silently drop an instantiation."""
    classes = {
        "A bias+relu": [_kgeom(_case(*FWD[s])) for s in ALL_SHAPES],
        "A residual / out=": [_kgeom(_case(*FWD[s])) for s in EPI_SHAPES],
        "A statistics": [_kgeom(_case(*FWD[s])) for s in STAT_SHAPES],
        "B plain / residual": [_dgeom(_case(*DGR[s])) for s in DGR],
        "B strided residual / BN backward / tail": [_dgeom(_case(*DGR[s])) for s in DG_EPI],
    }
    fwd_tiles = {(bn, bm, bk) for bn, bk, bm in TILE_CANDIDATES if bk > 1}
    x8_tiles = {(bm, bn) for bn, bk, bm in TILE_CANDIDATES if bk == 1}
    assert len(fwd_tiles) == 6 and len(x8_tiles) == 4
    for cls, geoms in classes.items():
        ran = {_igemm_inst(cand, *g) for cand in TILE_CANDIDATES for g in geoms}
        for bn, bm, bk in fwd_tiles:
            modes = {i[2] for i in ran if i[0] == "fwd" and (i[1], i[3], i[4]) == (bn, bm, bk)}
            assert modes >= {0, 1, 3}, (cls, bn, bm, bk)
        for bm, bn in x8_tiles:
            assert {i[3] for i in ran if i[0] == "x8" and i[1:3] == (bm, bn)} == {1, 3}, (cls, bm, bn)


# ----------------------------------------------------------------- C. weight-gradient candidates
def _wg_plan(c, cand, deterministic=False):
    """wgrad_launch's choices (conv_wgrad.hip) for a pinned (target blocks, depth): the k_conv_wgrad<TN, TK,
    BPT, C4, D3, AT, PW1, F32, PRO> template arguments, the split count and the last split's rows."""
    N, C, K, H, W, R, S = c.geom
    cdiv = lambda a, b: -(-a // b)
    cc = 4 if C <= 4 else (C + 7) // 8 * 8
    c4 = cc == 4
    M, Kg = c.M, R * S * cc
    P, Q = c.y.shape[2:]
    pw1 = R == 1 and S == 1 and c.stride == s1 and c.pad == p0 and (P, Q) == (H, W) and not c4
    TN, TK = (64 if K <= 64 else 128), (64 if (Kg <= 64 and not c4) else 128)
    tiles = cdiv(K, TN) * cdiv(Kg, TK)
    heur = 2048 if cc <= 8 else (768 if (M >= 400000 and (cc <= 64 or K <= 64)) else 384)   # _wgrad_blocks
    target = cand[0] or heur
    splits = 1 if deterministic else max(1, min(cdiv(target, tiles), cdiv(M, 512)))
    mps = cdiv(cdiv(M, splits), 64) * 64   # rows per split, rounded up to 64 pixels
    splits = cdiv(M, mps)
    bp = cand[1] or (32 if (tiles <= 16 and K >= 128) else 64)
    b = lambda v: "true" if v else "false"
    inst = [str(TN), str(TK), str(bp), b(c4), "false", "false", b(pw1), "false", "false"]
    return inst, splits, M - (splits - 1) * mps


def _check_wg(names, inst):
    ts = [_targs(n) for n in names if "k_conv_wgrad" in n]
    assert ts == [inst], (ts, inst, names)


def _wgrad(c, scale, bias=False):
    """``fn`` → (gw, gb) of one bf16 NO.conv2d_backward without input gradient, accumulated with ``scale`` into
    fresh copies of the case's non-zero accumulators."""
    from bigdl.ops import native_ops as NO
    xd, wd, gyd = _d(c.x), _d(c.w), _d(c.gy)
    G0, B0 = c.G0.to(dev), c.B0.to(dev)

    def fn():
        gw = G0.clone().permute(0, 3, 1, 2)
        gb = B0.clone() if bias else None
        gi = NO.conv2d_backward(gyd, xd, wd, c.stride, c.pad, (1, 1), 1, False, gw, gb, scale)
        assert gi is None
        return gw, gb
    return fn


def _check_acc(c, gw, gb, scale):
    """gw − G0 against scale·ref (the error relative to ‖scale·ref‖), likewise gb."""
    d = gw.double().cpu() - c.G0.double().permute(0, 3, 1, 2)
    _report("C", "gw", _rel(d, scale * c.gw), TOL_GW, strict=True)
    if gb is not None:
        _report("C", "gb", _rel(gb.double().cpu() - c.B0.double(), scale * c.gb), TOL_GB, strict=True)


# Splits are clamped to ⌈M / 512⌉.  N = 6 on 14×14 outputs: M = 1176 → 3 splits of ⌈392 / 64⌉·64 = 448 rows,
# the last 280: 7 / 5 k-tiles at depth 64 (the last of 24 rows), 14 / 9 at depth 32 — both parities of the two-stage
# pipeline.  Every candidate's target (≥ 256 blocks over ≤ 15 tiles) asks for more than 3, so all resolve to 3.
WGR = {
    # name: geometry, (TN, TK, PW1, C4), (splits, rows of the last split) for every candidate
    "pw_64x64": ((6, 64, 64, 14, 14, 1, 1, s1, p0), (64, 64, True, False), (3, 280)),
    "pw_64x128": ((6, 264, 64, 14, 14, 1, 1, s1, p0), (64, 128, True, False), (3, 280)),   # Kg = 264 = 2·128 + 8
    "pw_128x64": ((6, 64, 264, 14, 14, 1, 1, s1, p0), (128, 64, True, False), (3, 280)),   # K = 264 = 2·128 + 8
    "pw_128x128": ((6, 264, 264, 14, 14, 1, 1, s1, p0), (128, 128, True, False), (3, 280)),
    # gather: tiles_n and tiles_k both end in partial tiles (264 = 2·128 + 8, 576 = 4·128 + 64)
    "g_3x3": ((6, 64, 264, 14, 14, 3, 3, s1, p1), (128, 128, False, False), (3, 280)),
    "g_3x3s2": ((6, 64, 264, 27, 27, 3, 3, s2, p1), (128, 128, False, False), (3, 280)),   # 27 → 14 outputs
    "g_1x1s2": ((6, 64, 264, 27, 27, 1, 1, s2, p0), (128, 64, False, False), (3, 280)),    # pointwise, not PW1
    # one split: M = 351 = 5·64 + 31 (⌈351 / 512⌉ = 1)
    "g_3x3_1split": ((3, 64, 264, 13, 9, 3, 3, s1, p1), (128, 128, False, False), (1, 351)),
    # the only split is shorter than one k-tile at either depth: M = 49
    "pw_tiny": ((1, 64, 264, 7, 7, 1, 1, s1, p0), (128, 64, True, False), (1, 49)),
    "g_tiny": ((1, 64, 264, 7, 7, 3, 3, s1, p1), (128, 128, False, False), (1, 49)),
    # the RGB stem: 3 → 4 channels, 7×7 s2 p3, M = 3·15·15 = 675 → 2 splits of 384 rows, the last 291;
    # K = 136 = 128 + 8, Kg = 196 = 128 + 68; the C4 gradient is folded onto the KCRS accumulator
    "c4_stem": ((3, 3, 136, 30, 30, 7, 7, s2, (3, 3)), (128, 128, False, True), (2, 291)),
}


@wg_cands
@pytest.mark.parametrize("name", list(WGR))
def test_wgrad_accumulates_scaled_gradient(cand, name):
    geom, (TN, TK, pw1, c4), (splits, last) = WGR[name]
    c = _case(*geom)
    inst, sp, ls = _wg_plan(c, cand)
    # the case's comment, so a later change of the launcher's formula cannot silently empty the test
    assert (sp, ls) == (splits, last), (sp, ls)
    b = lambda v: "true" if v else "false"
    assert inst[:2] == [str(TN), str(TK)] and inst[3] == b(c4) and inst[6] == b(pw1), inst
    assert cand[1] == 0 or inst[2] == str(cand[1])
    bias = name == "pw_128x128"
    (gw, gb), names = _pinned(_wgrad(c, 2.0, bias), cand, "wg")
    _check_wg(names, inst)
    if c4:
        assert any("c4_wgrad_fold" in n for n in names), names
    _check_acc(c, gw, gb, 2.0)


def test_wgrad_split_edges_present():
    """Across part C: a 1-split case, a ≥ 3-split case with a partial last split, a case whose only split is
    shorter than one k-tile."""
    plans = {n: _wg_plan(_case(*WGR[n][0]), (0, 0)) for n in WGR}
    assert any(s == 1 and l >= 64 for _, s, l in plans.values())
    assert any(s >= 3 and l % 64 for _, s, l in plans.values())
    assert any(s == 1 and l < 64 for _, s, l in plans.values())
    for n in WGR:   # every shape's instantiation runs at both depths across the candidates
        assert {_wg_plan(_case(*WGR[n][0]), cnd)[0][2] for cnd in WG_ALL} == {"32", "64"}, n


@wg_cands
def test_wgrad_deterministic_is_one_split(cand):
    """bigdl.deterministic: one block per weight tile (no atomics), whatever split target is pinned — 3 splits
    otherwise on this shape; two runs are bit-identical."""
    from bigdl.utils import config
    c = _case(*WGR["g_3x3"][0])
    inst, sp, ls = _wg_plan(c, cand, deterministic=True)
    assert _wg_plan(c, cand)[1] == 3 and (sp, ls) == (1, 1176)
    fn = _wgrad(c, 2.0, True)
    config.set_property("bigdl.deterministic", True)
    try:
        (gw, gb), names = _pinned(fn, cand, "wg")
        (gw2, _), _ = _pinned(fn, cand, "wg")
    finally:
        config.set_property("bigdl.deterministic", False)
    _check_wg(names, inst)
    _check_acc(c, gw, gb, 2.0)
    assert torch.equal(gw, gw2)   # single-writer reduction: bit-reproducible


# ------------------------------------------- D. re-timing must not touch live statistics
def _retime(fn, cand):
    """Record ``fn``'s launches, then re-launch each recorded closure with ``cand`` under _TILE["retiming"], the
    way select_kernels' timing loop does: the kernel names of the re-launches."""
    from bigdl.ops import native_ops as NO
    rec = NO._TILE["record"] = {}
    try:
        fn()
    finally:
        NO._TILE["record"] = None
    torch.cuda.synchronize()
    launches = [f for k, f in rec.items() if _family(k) == "conv"]
    assert launches, list(rec)
    NO._TILE["retiming"] = True
    try:
        return _kernels(lambda: [f(cand) for f in launches])[1]
    finally:
        NO._TILE["retiming"] = False


def test_retiming_leaves_forward_replica_statistics():
    from bigdl.ops import native_ops as NO
    cand = (128, 64, 256)
    c = _case(*FWD["S3"])
    K, rep = c.geom[2], 2
    xd, wd, _ = _fwd_args(c)
    sd = torch.zeros(K, device=dev)
    buf = torch.zeros(2 * rep * K, device=dev)
    live = {}

    def fn():
        buf.zero_()
        NO.conv2d_forward_stats(xd, wd, None, c.stride, c.pad, shift=sd, sums=(buf, rep))
        torch.cuda.synchronize()
        live["sums"] = buf.clone()
    names = _retime(fn, cand)
    _check_conv(names, cand, _kgeom(c))
    assert float(live["sums"].abs().max()) > 0
    assert torch.equal(buf, live["sums"]), "a re-timed launch added into the live BN sums"


def test_retiming_leaves_dgrad_bn_backward_replicas():
    cand = (128, 1, 256)
    c = _case(*DGR["D1"])
    C, rep = c.geom[1], 2
    xb, sc, sh, mean, mask = _bn_input(c.x.shape, 6)
    buf = torch.zeros(2 * rep * C, device=dev)
    base = {"x": _d(xb), "mean": mean.to(dev), "scale": sc.to(dev), "shift": sh.to(dev), "sums": (buf, rep)}
    f = _bwd(c)
    live = {}

    def fn():
        buf.zero_()
        f(bn_fuse=dict(base))
        torch.cuda.synchronize()
        live["sums"] = buf.clone()
    names = _retime(fn, cand)
    _check_conv(names, cand, _dgeom(c))
    assert float(live["sums"].abs().max()) > 0
    assert torch.equal(buf, live["sums"]), "a re-timed launch added into the live BN-backward sums"
