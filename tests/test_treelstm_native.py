"""The BinaryTreeLSTM level kernels (ops/csrc/treelstm.hip) and the layer's native path against the leaf and
composer equations of ``bigdl/nn/layers/tree_lstm.py`` in plain torch fp64 on the host, with their
hand-written adjoint, one level at a time.

Part 1 (CPU) runs the oracle free against ``BinaryTreeLSTM(...).to(float64)``: 1e-12.  Part 2 runs single
levels teacher-forced as tests/test_rnn_oracle.py does (the children's h and the parents' gate gradients
reach the oracle as the device holds them in bf16; fp32 state runs free) with that file's bounds:
bf16 outputs 2^-8·|ref| + A·rms(ref), fp32-held outputs A·rms(ref).  A = 2e-5: this oracle in torch fp32
against itself in fp64 on the host at H 150 / K 300, 70 rows, is worst 4.4e-6·rms (composer backward gate
gradients; every forward output ≤ 9.9e-7), below 1e-5.  Part 3 runs the layer on whole batches and holds the native path to
2 × the error of the ``bigdl.treelstm.native=false`` device path against the fp64 layer (floor 2^-8·max|ref|).
Worst observed fractions are in profiles/treelstm_errors.txt.
"""
import pytest
import torch

from test_rnn_oracle import Draw, Guard, NO, close_bf16, close_f32, d, dev  # noqa: F401
from test_tree_lstm import TREE1, TREE2
from bigdl.ops.native_ops import _up

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64
sg = torch.sigmoid


# ------------------------------------------------------------------------------------------ the oracle
def leaf_fwd(x, Wc, bc, Wo=None, bo=None):
    c = x @ Wc.t() + bc
    o = sg(x @ Wo.t() + bo) if Wo is not None else torch.ones_like(c)
    return o * torch.tanh(c), c, o, torch.tanh(c)


def comp_fwd(lh, rh, lc, rc, Wl, bl, Wr, br):
    """→ h, c, act [n][G][H] (i, lf, rf, u[, o]), tanh c."""
    H = lh.shape[1]
    a = (lh @ Wl.t() + bl + rh @ Wr.t() + br).view(len(lh), -1, H)
    a = torch.cat([sg(a[:, :3]), torch.tanh(a[:, 3:4]), sg(a[:, 4:])], 1)
    c = a[:, 0] * a[:, 3] + a[:, 1] * lc + a[:, 2] * rc
    o = a[:, 4] if a.shape[1] == 5 else 1.0
    return o * torch.tanh(c), c, a, torch.tanh(c)


def comp_bwd(dh, dcp, a, tc, lc, rc):
    """dh, the parent's share of dc → gate gradients [n][G][H], dc (children take dc·lf, dc·rf and dg·W)."""
    i, lf, rf, u = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    o = a[:, 4] if a.shape[1] == 5 else torch.ones_like(i)
    dc = dcp + dh * o * (1 - tc * tc)
    dg = [dc * u * i * (1 - i), dc * lc * lf * (1 - lf), dc * rc * rf * (1 - rf), dc * i * (1 - u * u)]
    return torch.stack(dg + ([dh * tc * o * (1 - o)] if a.shape[1] == 5 else []), 1), dc


def leaf_bwd(dh, dcp, o, tc):
    return dcp + dh * o * (1 - tc * tc), dh * tc * o * (1 - o)


def tree_oracle(P, x, trees, gy):
    """Whole batch, free-running: → out (B, N, H), gx, {parameter: gradient}."""
    from bigdl.nn.layers.tree_lstm import _schedule
    (B, L, _), N, H, go = x.shape, trees.shape[1], P["left_weight"].shape[1], "leaf_o_weight" in P
    leaves, levels = _schedule(trees)
    Hs, Cs = torch.zeros(B * N, H, dtype=x.dtype), torch.zeros(B * N, H, dtype=x.dtype)
    nl, xr = torch.tensor([l[0] for l in leaves]), torch.tensor([l[1] * L + l[2] - 1 for l in leaves])
    xl = x.reshape(B * L, -1)[xr]
    Hs[nl], Cs[nl], lo, ltc = leaf_fwd(xl, P["leaf_c_weight"], P["leaf_c_bias"], P.get("leaf_o_weight"), P.get("leaf_o_bias"))
    saves = []
    for lvl in levels:
        me, lk, rk = torch.tensor(lvl).t()
        Hs[me], Cs[me], a, tc = comp_fwd(Hs[lk], Hs[rk], Cs[lk], Cs[rk], P["left_weight"], P["left_bias"],
                                         P["right_weight"], P["right_bias"])
        saves.append((me, lk, rk, a, tc))
    dH, dC = gy.reshape(B * N, H).clone(), torch.zeros(B * N, H, dtype=x.dtype)
    g = {k: torch.zeros_like(v) for k, v in P.items()}
    for me, lk, rk, a, tc in reversed(saves):
        dg, dc = comp_bwd(dH[me], dC[me], a, tc, Cs[lk], Cs[rk])
        dg = dg.reshape(len(me), -1)
        for s, k, f in (("left", lk, 1), ("right", rk, 2)):
            dH[k] += dg @ P[f"{s}_weight"]
            dC[k] = dc * a[:, f]
            g[f"{s}_weight"] += dg.t() @ Hs[k]
            g[f"{s}_bias"] += dg.sum(0)
    gx = torch.zeros(B * L, x.shape[2], dtype=x.dtype)
    for nm, da in zip(("c", "o") if go else ("c",), leaf_bwd(dH[nl], dC[nl], lo, ltc)):
        g[f"leaf_{nm}_weight"], g[f"leaf_{nm}_bias"] = da.t() @ xl, da.sum(0)
        gx[xr] += da @ P[f"leaf_{nm}_weight"]
    return Hs.view(B, N, H), gx.view(x.shape), g


def _layer_run(m, x, trees, gy):
    from bigdl.utils.table import Table
    m.training()
    y, gi = m.forward(Table(x, trees)), m.backward(Table(x, trees), gy)
    return y, gi[1], {w: getattr(m, g) for w, g in m._param_slots}


@pytest.mark.parametrize("gate", (True, False))
def test_oracle_matches_fp64_layer(gate):
    from bigdl.nn import BinaryTreeLSTM
    torch.manual_seed(3)
    m = BinaryTreeLSTM(6, 5, gate_output=gate).to(dtype=f64)
    trees, x, gy = torch.tensor([TREE1, TREE2], dtype=f64), torch.randn(2, 6, 6, dtype=f64), torch.randn(2, 13, 5, dtype=f64)
    y, gx, grads = _layer_run(m, x, trees, gy)
    oy, ogx, og = tree_oracle({w: getattr(m, w) for w, _ in m._param_slots}, x, trees, gy)
    for a, b in [(y, oy), (gx, ogx)] + [(grads[k], og[k]) for k in og]:
        assert float((a - b).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------- GPU: single levels
def _rows(n):
    """Level rows of n nodes: the first half left children, the rest right children, each padded to 32."""
    nl = (n + 1) // 2
    side = [0] * nl + [-1] * (_up(nl, 32) - nl) + [1] * (n - nl) + [-1] * (_up(n - nl, 32) - (n - nl))
    return torch.tensor(side)


def _level_case(NO, mode, go, H, n, K=10):
    part, tag = "T", f"{mode}:go{int(go)}:H{H}:n{n}:K{K}"
    r = Draw(100 * H + n + K + len(mode))
    G, GL, Hp = (5 if go else 4), (2 if go else 1), _up(H, 8)
    leafm, bwd = mode.startswith("leaf"), mode.endswith("bwd")
    side = torch.tensor([(-1 if j % 3 == 2 else j % 2) for j in range(_up(n, 32))]) if leafm else _rows(n)
    if leafm:
        side[n:] = -1
    rows, live, nlive = len(side), side >= 0, int((side >= 0).sum())
    nn = 3 * nlive + 2
    perm = torch.randperm(nn, generator=r.g)
    node = torch.full((rows,), -1, dtype=torch.int64)
    lk, rk = node.clone(), node.clone()
    node[live], lk[live], rk[live] = perm[:nlive], perm[nlive:2 * nlive], perm[2 * nlive:3 * nlive]
    prow = torch.where(live & (torch.arange(rows) % 5 != 4), rows + torch.arange(rows), -1) if bwd else node * 0 - 1
    plan = torch.stack([node, lk, rk, prow, side.clamp(min=0)]).to(torch.int32).cuda()
    W = {k: r.w(G * H, H) for k in ("left", "right")} | {k: r.w(H, K) for k in ("c", "o")[:GL]}
    b = {k: r.n(v.shape[0], dt=f32) for k, v in W.items()}
    pk = NO.treelstm_pack(H, K, *[dev(t) for t in (W["left"], W["right"], b["left"], b["right"], W["c"], b["c"])],
                          *([dev(W["o"]), dev(b["o"])] if go else []))
    g = Guard()
    h0, c0 = r.h(nn, H), r.n(nn, H, dt=f32)
    hb, cb = g.new((nn, H), bf, h0), g.new((nn, H), f32, c0)
    act, tc, nd = g.new((rows, 1 if leafm else G, H), f32), g.new((rows, H), f32), node[live]
    if not bwd:
        x, xs = r.n(rows, K), g.new((rows, _up(K, 8) if leafm else 2 * Hp), bf)
        before = {k: v.clone() for k, v in (("act", act), ("tc", tc), ("xs", xs))}
        NO.treelstm_level(mode, go, plan, 0, rows, H, K, dev(x) if leafm else hb, pk["wl" if leafm else "wc"],
                          pk["bl" if leafm else "bc"], c=cb, h=hb, act=act if (go or not leafm) else None, tc=tc, xs=xs)
        if leafm:
            rh, rc, ra, rtc = leaf_fwd(d(x)[live], d(W["c"]), d(b["c"]), *((d(W["o"]), d(b["o"])) if go else ()))
            ra, ops_ = ra[:, None], [(d(x)[live], 0)]
        else:
            rh, rc, ra, rtc = comp_fwd(d(h0)[lk[live]], d(h0)[rk[live]], d(c0)[lk[live]], d(c0)[rk[live]],
                                       d(W["left"]), d(b["left"]), d(W["right"]), d(b["right"]))
            ops_ = [(d(h0)[lk[live]], 0), (d(h0)[rk[live]], Hp)]
        close_bf16(part, tag + ":h", hb[nd.cuda()], rh)
        close_f32(part, tag + ":c", cb[nd.cuda()], rc)
        if go or not leafm:
            close_f32(part, tag + ":act", act[live.cuda()], ra)
        close_f32(part, tag + ":tc", tc[live.cuda()], rtc)
        for o, off in ops_:
            assert torch.equal(xs[live.cuda()][:, off:off + o.shape[1]].double().cpu(), o), tag
        rest = torch.ones(nn, dtype=torch.bool).index_fill(0, nd, False)
        assert torch.equal(hb.cpu()[rest], h0[rest]) and torch.equal(cb.cpu()[rest], c0[rest]), tag
        out = {"act": act, "tc": tc, "xs": xs}
    else:
        # the parents' saves, rows [rows, 2·rows) of the composer space, as the device holds them
        DG = torch.zeros(2 * rows, G, Hp, dtype=bf)
        DG[rows:, :, :H] = r.n(rows, G, H)
        pact, pdc, gy = r.sig(2 * rows, G, H), r.n(2 * rows, H, dt=f32), r.n(nn, H)
        a_own = torch.cat([r.sig(rows, 3, H), torch.tanh(r.n(rows, 1, H, dt=f32)), r.sig(rows, G - 4, H)], 1)
        a_own = a_own[:, -1:] if leafm else a_own
        tcv = torch.tanh(r.n(rows, H, dt=f32))
        act.copy_(a_own), tc.copy_(tcv)
        dg, dc = g.new((rows, GL if leafm else G, Hp), bf), g.new((rows, H), f32)
        dgall = dg if leafm else g.new((2 * rows, G, Hp), bf, DG)
        before = {"dg": (dgall[:rows] if not leafm else dg).clone(), "dc": dc.clone()}
        NO.treelstm_level(mode, go, plan, 0, rows, H, K, dev(DG) if leafm else dgall, pk["wt"], c=cb,
                          act=act if (go or not leafm) else None, tc=tc, gy=dev(gy), pact=dev(pact), pdc=dev(pdc),
                          dg=dgall if not leafm else dg, dc=None if leafm else dc)
        has = (prow[live] >= 0).double()[:, None]
        pr, sd = prow[live].clamp(min=0), side[live]
        A = d(DG)[pr][:, :, :H].reshape(nlive, -1)
        dh = d(gy)[nd] + has * torch.where(sd[:, None] == 0, A @ d(W["left"]), A @ d(W["right"]))
        dcp = has * d(pdc)[pr] * d(pact)[pr, 1 + sd]
        if leafm:
            ref = torch.stack(leaf_bwd(dh, dcp, d(a_own)[live][:, 0] if go else 1.0, d(tcv)[live])[:GL], 1)
        else:
            ref, rdc = comp_bwd(dh, dcp, d(a_own)[live], d(tcv)[live], d(c0)[lk[live]], d(c0)[rk[live]])
            close_f32(part, tag + ":dc", dc[live.cuda()], rdc)
        got = (dg if leafm else dgall[:rows])
        close_bf16(part, tag + ":dg", got[live.cuda()][:, :, :H], ref)
        out = {"dg": got, "dc": dc}
    for k, v in before.items():   # pad rows keep the sentinel
        assert torch.equal(out[k][(~live).cuda()], v[(~live).cuda()]), (tag, k)
    g.check()


@pytest.mark.gpu
@pytest.mark.parametrize("H", (8, 22, 40, 150))
@pytest.mark.parametrize("go", (True, False))
@pytest.mark.parametrize("mode", ("leaf_fwd", "comp_fwd", "comp_bwd", "leaf_bwd"))
def test_level_steps(NO, mode, go, H):
    for n in (1, 32, 33, 70):
        for K in ((10, 40) if mode == "leaf_fwd" else (10,)):
            _level_case(NO, mode, go, H, n, K)


# ------------------------------------------------------------------------------------- GPU: the layer
def _chain(n):
    """Left-deep tree of n leaves: one composer row per level."""
    rows = [[0, 0, k + 1] for k in range(n)]
    top = 1
    for k in range(1, n):
        rows.append([top, k + 1, 0])
        top = n + k
    rows[-1][2] = -1
    return rows


def _bigdl():
    from bigdl import ops
    from bigdl.nn import BinaryTreeLSTM
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.utils.table import Table
    Engine.init(device="cuda:0")
    return ops, BinaryTreeLSTM, config, Table


BATCHES = {"doc": [TREE1, TREE2], "chain": [_chain(6)], "single": [[[0, 0, 1]]],
           "balanced": [[[0, 0, 1], [0, 0, 2], [0, 0, 3], [0, 0, 4], [1, 2, 0], [3, 4, 0], [5, 6, -1]]] * 40}


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", ((10, 22), (300, 150)))
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_layer_native_vs_fp64(batch, sizes):
    ops, BinaryTreeLSTM, config, Table = _bigdl()
    (IN, H), trees = sizes, torch.tensor(BATCHES[batch], dtype=f32)
    B, N, L = trees.shape[0], trees.shape[1], int(trees[..., 2].max())
    ref = BinaryTreeLSTM(IN, H)
    for w, _ in ref._param_slots:
        getattr(ref, w).copy_(getattr(ref, w).to(bf))
    gpu = ref.cloneModule().to(device="cuda")
    x, gy = torch.randn(B, L, IN).to(bf), torch.randn(B, N, H).to(bf)
    want = _layer_run(ref.to(dtype=f64), x.double(), trees.double(), gy.double())
    res = {}
    for native in (False, True):
        config.set_property("bigdl.treelstm.native", native)
        try:
            gpu.zeroGradParameters()
            ops.reset_fallbacks()
            y, gx, gr = _layer_run(gpu, x.cuda(), trees.cuda(), gy.cuda())
            res[native] = [y, gx] + [gr[w].clone() for w, _ in gpu._param_slots]
            assert (ops.fallback_counts() == {}) == native, ops.fallback_counts()
        finally:
            config.set_property("bigdl.treelstm.native", True)
    assert not res[True][0][(trees[..., 0] == -1).cuda()].any()
    names = ["out", "gx"] + [w for w, _ in gpu._param_slots]
    for nm, nat, tor, w in zip(names, res[True], res[False], [want[0], want[1]] + [want[2][k] for k in names[2:]]):
        e_nat, e_tor = float((d(nat) - w).abs().max()), float((d(tor) - w).abs().max())
        bound = max(2 * e_tor, 2.0 ** -8 * float(w.abs().max()))
        print(f"[treelstm] part=W what={batch}:{IN}x{H}:{nm} native={e_nat:.3e} torch={e_tor:.3e} frac={e_nat / bound if bound else 0:.3e}")
        assert e_nat <= bound, (nm, e_nat, e_tor)
    # a second pass accumulates; inference output is bit-equal to training output
    _layer_run(gpu, x.cuda(), trees.cuda(), gy.cuda())
    for w, g in gpu._param_slots:
        one = res[True][2 + names[2:].index(w)]
        # fp32 atomic sums in another order; an overwrite would miss by max|one|
        assert float((getattr(gpu, g) - 2 * one).abs().max()) <= 1e-3 * float(one.abs().max()), w
    gpu.evaluate()
    assert torch.equal(gpu.forward(Table(x.cuda(), trees.cuda())), res[True][0])


@pytest.mark.gpu
@pytest.mark.parametrize("why", ("property", "odd"))
def test_ineligible_takes_torch_path(why):
    ops, BinaryTreeLSTM, config, Table = _bigdl()
    m = BinaryTreeLSTM(10, 21 if why == "odd" else 22).to(device="cuda")
    trees, x = torch.tensor([TREE1, TREE2], dtype=f32).cuda(), torch.randn(2, 6, 10).to(bf).cuda()
    config.set_property("bigdl.treelstm.native", why != "property")
    try:
        ops.reset_fallbacks()
        y = m.forward(Table(x, trees))
        assert [k[0] for k in ops.fallback_counts()] == ["treelstm_forward"]
        with torch.no_grad():
            assert torch.equal(y, m._forward(Table(x, trees)))
    finally:
        config.set_property("bigdl.treelstm.native", True)
        ops.reset_fallbacks()
