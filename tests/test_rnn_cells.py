"""RnnCell and LSTMPeephole on the fused step kernels (rnn_step.hip cells 6-9, ``bigdl_rnn_seq_*``,
``bigdl_lstmp_seq_*``, ``bigdl_peephole_grad``) against a torch fp64 oracle written from ``DL/nn/RNN.scala``,
``DL/nn/LSTMPeephole.scala`` (gates i, f, g, o; i / f peep at c₋₁, o at c) and the BPTT of ``Recurrent.scala``.
Teacher forcing, guard bands, draws, shapes and the bf16 / fp32 / bf16x3 bounds are those of tests/test_rnn_oracle.py;
``peephole_grad``: per element n·2⁻²⁴·Σ|term| (n = B·T) against fp64 of the same DG.  The 2e-5 allowance stays: this
oracle in torch fp32 against itself in fp64 on the host, free-running at H 264, B 33, T 3, is worst at the
LSTMPeephole DG, 4.8e-6·rms(ref) < 1e-5.  Every figure, and the worst fraction of each bound per part on an MI355X:
profiles/rnn_cells_errors.txt.
"""
import pytest
import torch

from test_rnn_oracle import (NO, Draw, Guard, SHAPES_H, SHAPES_M, TS, _hprev, _maxdiff, bf, close_bf16,  # noqa: F401
                             close_f32, close_x3, d, dev, f32, f64, tr)

ACT = {"Tanh": (torch.tanh, lambda h: 1 - h * h), "ReLU": (torch.relu, lambda h: (h > 0).to(h.dtype)),
       "Sigmoid": (torch.sigmoid, lambda h: h * (1 - h))}
KINDS = tuple(ACT)


def rnn_fwd(x2, h0, bh, U, kind, forced=None):
    out = []
    for t in range(x2.shape[1]):
        hp = h0 if t == 0 else (forced[:, t - 1] if forced is not None else out[-1])
        out.append(ACT[kind][0](x2[:, t] + bh + hp @ U.t()))
    return torch.stack(out, 1)


def rnn_bwd(gy, U, hs, kind, forced=None):
    T = gy.shape[1]
    DG = [None] * T
    for t in range(T - 1, -1, -1):
        dh = gy[:, t]
        if t + 1 < T:
            dh = dh + (forced[:, t + 1] if forced is not None else DG[t + 1]) @ U
        DG[t] = dh * ACT[kind][1](hs[t])
    return torch.stack(DG, 1)


def lstmp_cell_fwd(pre, c_prev, P):
    """pre [M][4H] (i, f, g, o), P [3][H] (p_i, p_f, p_o) → h, c, acts [M][4H], tanh c."""
    H = pre.shape[1] // 4
    i, f = torch.sigmoid(pre[:, :H] + P[0] * c_prev), torch.sigmoid(pre[:, H:2 * H] + P[1] * c_prev)
    g = torch.tanh(pre[:, 2 * H:3 * H])
    c = f * c_prev + i * g
    o, tc = torch.sigmoid(pre[:, 3 * H:] + P[2] * c), torch.tanh(c)
    return o * tc, c, torch.cat([i, f, g, o], 1), tc


def lstmp_cell_bwd(dh, acts, tc, c_prev, dc_next, P):
    i, f, g, o = acts.split(tc.shape[1], 1)
    da_o = dh * tc * o * (1 - o)
    dc = dh * o * (1 - tc * tc) + dc_next + da_o * P[2]
    da_i, da_f = dc * g * i * (1 - i), dc * c_prev * f * (1 - f)
    return torch.cat([da_i, da_f, dc * i * (1 - g * g), da_o], 1), dc * f + da_i * P[0] + da_f * P[1]


def lstmp_fwd(x2, h0, c0, U, P, forced=None):
    c = torch.zeros_like(h0) if c0 is None else c0
    out, cs, acts, tcs = [], [], [], []
    for t in range(x2.shape[1]):
        hp = h0 if t == 0 else (forced[:, t - 1] if forced is not None else out[-1])
        h, c, a, tc = lstmp_cell_fwd(x2[:, t] + hp @ U.t(), c, P)
        out.append(h), cs.append(c), acts.append(a), tcs.append(tc)
    return torch.stack(out, 1), torch.stack(cs), torch.stack(acts), torch.stack(tcs)


def lstmp_bwd(gy, U, P, acts, tcs, cs, c0, forced=None):
    T = gy.shape[1]
    DG, dc = [None] * T, torch.zeros_like(gy[:, 0])
    for t in range(T - 1, -1, -1):
        dh = gy[:, t]
        if t + 1 < T:
            dh = dh + (forced[:, t + 1] if forced is not None else DG[t + 1]) @ U
        c_prev = cs[t - 1] if t > 0 else (torch.zeros_like(dc) if c0 is None else c0)
        DG[t], dc = lstmp_cell_bwd(dh, acts[t], tcs[t], c_prev, dc, P)
    return torch.stack(DG, 1), dc


def peep_terms(DG, cs, c0):
    """[3][B][T][H]: the summands of the three CMul gradients."""
    H = cs.shape[2]
    c = cs.transpose(0, 1)
    cp = torch.cat([(torch.zeros_like(c[:, 0]) if c0 is None else c0).unsqueeze(1), c[:, :-1]], 1)
    return torch.stack([DG[..., :H] * cp, DG[..., H:2 * H] * cp, DG[..., 3 * H:] * c])


@pytest.mark.parametrize("kind", KINDS + ("peephole",))
def test_oracle_reproduces_fp64_recurrent_layers(kind):
    import bigdl.nn as nn
    from bigdl.utils.table import T as Tbl
    B, T, IN, H = 3, 3, 5, 8
    g = torch.Generator().manual_seed(23)
    x, gy = torch.randn(B, T, IN, generator=g, dtype=f64), torch.randn(B, T, H, generator=g, dtype=f64)
    h0, c0 = torch.tanh(torch.randn(B, H, generator=g, dtype=f64)), torch.randn(B, H, generator=g, dtype=f64)
    peep = kind == "peephole"
    rec = nn.Recurrent().add(nn.LSTMPeephole(IN, H) if peep else nn.RnnCell(IN, H, getattr(nn, kind)())).to(dtype=f64)
    rec.training()
    rec.setHiddenState(Tbl(h0.clone(), c0.clone()) if peep else h0.clone())
    y = rec.forward(x)
    rec.zeroGradParameters()
    gi = rec.backward(x, gy)
    W, gW = rec.parameters()
    gh = rec.getGradHiddenState()
    x2 = x @ W[0].t() + W[1]
    if peep:
        U, P = torch.cat(W[2:6]), torch.stack(W[6:9])
        out, cs, acts, tcs = lstmp_fwd(x2, h0, c0, U, P)
        DG, gc = lstmp_bwd(gy, U, P, acts, tcs, cs, c0)
        figs = {"gc": _maxdiff(gh[1], gc), "gU": _maxdiff(torch.cat(gW[2:6]), torch.einsum("btg,bth->gh", DG, _hprev(h0, out))),
                "gp": _maxdiff(torch.stack(gW[6:9]), peep_terms(DG, cs, c0).sum((1, 2)))}
    else:
        U = W[2]
        out = rnn_fwd(x2, h0, W[3], U, kind)
        DG = rnn_bwd(gy, U, out.transpose(0, 1), kind)
        figs = {"gU": _maxdiff(gW[2], torch.einsum("btg,bth->gh", DG, _hprev(h0, out))), "gb": _maxdiff(gW[3], DG.sum((0, 1)))}
    figs.update({"y": _maxdiff(y, out), "gi": _maxdiff(gi, DG @ W[0]), "gh": _maxdiff(gh[0], DG[:, 0] @ U)})
    for k, v in figs.items():
        print(f"[rnn-oracle] part=cpu what={kind}:{k} maxdiff={v:.3e}")
        assert v <= 1e-12, (k, v)


def _step_case(NO, cell, H, M, kind="Tanh", null=False):
    part, tag = "S", f"cell{cell}:H{H}:M{M}:{kind}" + (":null" if null else "")
    r, g = Draw(1000 * cell + 10 * H + M), Guard()
    hp, P, cp = r.h(M, H), r.n(3, H, dt=f32), None if null else r.n(M, H, dt=f32)
    z = lambda t: 0 if t is None else d(t)  # noqa: E731
    if cell == 6:
        xg, U, bh = r.n(M, H), r.w(H, H), None if null else r.n(H, dt=f32)
        h, hs = g.new((M, H), bf), g.new((M, H), f32)
        NO.rnn_step("rnn_fwd", dev(hp), dev(U), M, H, H, xg=dev(xg), bh=dev(bh), h_out=h, s0=hs, act_kind=kind)
        ref = ACT[kind][0](d(xg) + z(bh) + d(hp) @ d(U).t())
        got = [(close_bf16, "h", h, ref), (close_f32, "hs", hs, ref)]
    elif cell == 7:
        dan, Ut, gy, hs = r.n(M, H, scale=0.5), r.w(H, H), r.n(M, H), ACT[kind][0](r.n(M, H, dt=f32))
        dg = g.new((M, H), bf)
        NO.rnn_step("rnn_bwd", dev(dan), dev(Ut), M, H, H, gy=dev(gy), s0=dev(hs), dg=dg, act_kind=kind)
        got = [(close_bf16, "da", dg, (d(gy) + d(dan) @ d(Ut).t()) * ACT[kind][1](d(hs)))]
    elif cell == 8:
        xg, Ug = r.n(M, 4 * H), [r.w(H, H) for _ in range(4)]
        h, c, act, tc = g.new((M, H), bf), g.new((M, H), f32), g.new((M, 4 * H), f32), g.new((M, H), f32)
        NO.rnn_step("lstmp_fwd", dev(hp), [dev(u) for u in Ug], M, H, H, xg=dev(xg), peep=dev(P), c_prev=dev(cp),
                    h_out=h, c_out=c, act=act, tc=tc)
        rh, rc, ra, rtc = lstmp_cell_fwd(d(xg) + d(hp) @ d(torch.cat(Ug)).t(), z(cp), d(P))
        got = [(close_bf16, "h", h, rh), (close_f32, "c", c, rc), (close_f32, "tanh_c", tc, rtc)]
        got += [(close_f32, "act_" + nm, act[:, k * H:(k + 1) * H], ra[:, k * H:(k + 1) * H]) for k, nm in enumerate("ifgo")]
    else:
        dgn, Ut, gy, gcn = r.n(M, 4 * H, scale=0.5), r.w(H, 4 * H), r.n(M, H), None if null else r.n(M, H, dt=f32)
        acts = torch.cat([r.sig(M, H), r.sig(M, H), torch.tanh(r.n(M, H, dt=f32)), r.sig(M, H)], 1)
        tc = torch.tanh(r.n(M, H, dt=f32))
        dg, dcp = g.new((M, 4 * H), bf), g.new((M, H), f32)
        NO.rnn_step("lstmp_bwd", dev(dgn), dev(Ut), M, 4 * H, H, peep=dev(P), c_prev=dev(cp), act=dev(acts), tc=dev(tc),
                    gy=dev(gy), gc_next=dev(gcn), dg=dg, dc_prev=dcp)
        rdg, rdc = lstmp_cell_bwd(d(gy) + d(dgn) @ d(Ut).t(), d(acts), d(tc), z(cp), z(gcn), d(P))
        got = [(close_f32, "dc_prev", dcp, rdc)]
        got += [(close_bf16, "dg_" + nm, dg[:, k * H:(k + 1) * H], rdg[:, k * H:(k + 1) * H]) for k, nm in enumerate("ifgo")]
    g.check()
    for fn, nm, a, b in got:
        fn(part, f"{tag}:{nm}", a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("H", SHAPES_H)
@pytest.mark.parametrize("cell", (6, 7, 8, 9))
def test_step_cells(NO, cell, H):
    for k, M in enumerate(SHAPES_M):
        _step_case(NO, cell, H, M, KINDS[k % 3])
    if H == 24 and cell != 7:  # null bias (cell 6), null c_prev (8), null c_prev and gc_next (9)
        _step_case(NO, cell, 24, 17, null=True)


def _rnn_case(NO, kind, B, T, H, dt=bf):
    part, tag = "R" if dt == bf else "F", f"rnn:{kind}:H{H}:B{B}:T{T}"
    r, g = Draw(31000 + 100 * H + 4 * B + T, dt=dt), Guard()
    v = dict(x2=r.n(B, T, H), h0=r.h(B, H), bh=r.n(H, dt=f32), U=r.w(H, H), gy=r.n(B, T, H))
    fwd, bwd = (NO.rnn_seq_forward32, NO.rnn_seq_backward32) if dt == f32 else (NO.rnn_seq_forward, NO.rnn_seq_backward)
    o = dict(out=g.new((B, T, H), dt), hs=g.new((T, B, H), f32), DG=g.new((B, T, H), dt), inf=g.new((B, T, H), dt))
    args = [dev(v[k]) for k in ("x2", "h0", "bh", "U")]
    fwd(*args, o["out"], o["hs"], kind)
    fwd(*args, o["inf"], None, kind)
    bwd(dev(v["gy"]), dev(tr(v["U"])), o["hs"], o["DG"], kind)
    g.check()
    assert torch.equal(o["inf"].view(torch.uint8), o["out"].view(torch.uint8)), "inference != training forward"
    out = rnn_fwd(d(v["x2"]), d(v["h0"]), d(v["bh"]), d(v["U"]), kind, forced=d(o["out"]))
    rDG = rnn_bwd(d(v["gy"]), d(v["U"]), out.transpose(0, 1), kind, forced=d(o["DG"]))
    cb, cf = (close_bf16, close_f32) if dt == bf else (close_x3, close_x3)
    for t in range(T):
        cb(part, f"{tag}:out[{t}]", o["out"][:, t], out[:, t])
        cf(part, f"{tag}:hs[{t}]", o["hs"][t], out[:, t])
        cb(part, f"{tag}:DG[{t}]", o["DG"][:, t], rDG[:, t])


@pytest.mark.gpu
@pytest.mark.parametrize("H", SHAPES_H)
@pytest.mark.parametrize("kind", KINDS)
def test_rnn_sequence(NO, kind, H):
    for B in SHAPES_M:
        for T in TS:
            _rnn_case(NO, kind, B, T, H)


def _lstmp_case(NO, B, T, H, dt=bf, null_c=False):
    part, tag = "P" if dt == bf else "F", f"lstmp:H{H}:B{B}:T{T}" + (":c0=None" if null_c else "")
    r, g = Draw(41000 + 100 * H + 4 * B + T, dt=dt), Guard()
    x2, h0, c0, gy = r.n(B, T, 4 * H), r.h(B, H), None if null_c else r.n(B, H, dt=f32), r.n(B, T, H)
    Ug, P = [r.w(H, H) for _ in range(4)], r.n(3, H, dt=f32)
    x3 = dt == f32
    fwd, bwd = (NO.lstmp_seq_forward32, NO.lstmp_seq_backward32) if x3 else (NO.lstmp_seq_forward, NO.lstmp_seq_backward)
    o = dict(out=g.new((B, T, H), dt), cs=g.new((T, B, H), f32), acts=g.new((T, B, 4 * H), f32), tcs=g.new((T, B, H), f32),
             DG=g.new((B, T, 4 * H), dt), gc=g.new((B, H), f32), inf=g.new((B, T, H), dt), cbuf=g.new((2, B, H), f32))
    args = [dev(x2), dev(h0), dev(c0), [dev(u) for u in Ug], dev(P)]
    fwd(*args, o["out"], o["cs"], o["acts"], o["tcs"], None)
    fwd(*args, o["inf"], None, None, None, o["cbuf"])
    bwd(dev(gy), dev(tr(torch.cat(Ug))), dev(P), o["acts"], o["tcs"], o["cs"], dev(c0), o["DG"], o["gc"])
    gp = [g.new((H,), f32, init=torch.zeros(H)) for _ in range(6)]
    NO.peephole_grad(o["DG"], o["cs"], dev(c0), *gp[:3])
    NO.peephole_grad(o["DG"], o["cs"], dev(c0), *gp[3:])
    g.check()
    assert torch.equal(o["inf"].view(torch.uint8), o["out"].view(torch.uint8)), "inference != training forward"
    assert torch.equal(o["cbuf"][(T - 1) % 2], o["cs"][T - 1]), "inference c != training c"
    assert all(torch.equal(a, b) for a, b in zip(gp[:3], gp[3:])), "peephole_grad: two runs differ"
    U, P = d(torch.cat(Ug)), d(P)
    out, cs, acts, tcs = lstmp_fwd(d(x2), d(h0), d(c0), U, P, forced=d(o["out"]))
    rDG, rgc = lstmp_bwd(d(gy), U, P, acts, tcs, cs, d(c0), forced=d(o["DG"]))
    cb, cf = (close_x3, close_x3) if x3 else (close_bf16, close_f32)
    for t in range(T):
        cb(part, f"{tag}:out[{t}]", o["out"][:, t], out[:, t])
        cf(part, f"{tag}:cs[{t}]", o["cs"][t], cs[t])
        cf(part, f"{tag}:tcs[{t}]", o["tcs"][t], tcs[t])
        for k, nm in enumerate("ifgo"):
            sl = slice(k * H, (k + 1) * H)
            cf(part, f"{tag}:acts_{nm}[{t}]", o["acts"][t][:, sl], acts[t][:, sl])
            cb(part, f"{tag}:DG_{nm}[{t}]", o["DG"][:, t, sl], rDG[:, t, sl])
    cf(part, f"{tag}:gc", o["gc"], rgc)
    terms = peep_terms(d(o["DG"]), d(o["cs"]), d(c0))
    err, bound = (d(torch.stack(gp[:3])) - terms.sum((1, 2))).abs(), B * T * 2.0 ** -24 * terms.abs().sum((1, 2))
    print(f"[rnn-oracle] part={part} what={tag}:gp frac={float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("H", SHAPES_H)
def test_lstmp_sequence(NO, H):
    for B in SHAPES_M:
        for T in TS:
            _lstmp_case(NO, B, T, H)
    if H == 24:
        _lstmp_case(NO, 17, 3, 24, null_c=True)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 17))
@pytest.mark.parametrize("H", (8, 40))
def test_sequences_fp32(NO, H, B):
    _rnn_case(NO, "Tanh", B, 3, H, f32)
    _lstmp_case(NO, B, 3, H, f32)


@pytest.mark.gpu
@pytest.mark.parametrize("compute", ("bf16", "fp32"))
@pytest.mark.parametrize("cell", ("rnn", "lstmp"))
def test_layers_native_vs_fp64(cell, compute):
    import bigdl.nn as nn
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    config.set_property("bigdl.compute.dtype", compute)
    Engine.init(device="cuda:0")
    Engine.set_compute_dtype(compute)
    try:
        torch.manual_seed(0)
        B, T, IN, H = 17, 3, 24, 40
        ref = nn.Recurrent().add(nn.RnnCell(IN, H, nn.Tanh()) if cell == "rnn" else nn.LSTMPeephole(IN, H))
        gpu = ref.cloneModule().to(device="cuda")
        x, gy = torch.randn(B, T, IN), torch.randn(B, T, H)
        res = []
        for m, cv in ((ref.to(dtype=f64), torch.Tensor.double), (gpu, torch.Tensor.cuda)):
            m.training()
            y, tag = m.forward(cv(x)), m._rec[0]
            m.zeroGradParameters()
            res.append([y, m.backward(cv(x), cv(gy))] + m.parameters()[1])
        assert tag == cell, tag
        for k, (b, a) in enumerate(zip(*res)):
            a = a.double().cpu()
            if compute == "fp32":  # tolerances of the LSTM layer tests: test_rnn_fp32.py 1e-4, test_native_gemm_rnn.py 5e-2
                assert float((a - b).abs().max() / (b.abs().max() + 1e-12)) < 1e-4, k
            else:
                torch.testing.assert_close(a, b, rtol=5e-2, atol=5e-2 * (float(b.abs().max()) if k >= 2 else 1.0))
        config.set_property("bigdl.rnn.nativeCells", False)
        gpu.forward(x.cuda())
        assert gpu._rec[0] == "generic", gpu._rec[0]
    finally:
        config.set_property("bigdl.rnn.nativeCells", True)
        Engine.set_compute_dtype("bf16")
        config.set_property("bigdl.compute.dtype", "auto")
