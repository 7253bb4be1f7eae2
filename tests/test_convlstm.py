"""The ConvLSTMPeephole step kernels (convlstm.hip), their whole-sequence launchers and the layer path built
on them, against a torch fp64 evaluation of ``ConvLSTMPeephole.step`` (``DL/nn/ConvLSTMPeephole.scala:93-230``)
with ``F.conv2d`` in fp64.  Gate blocks (i, f, o, g); p_i, p_f on c₋₁, p_o on c.

Machinery (``Draw``, ``Guard``, ``close_bf16``, ``close_f32``, the bounds) and the teacher-forcing convention
are those of tests/test_rnn_oracle.py: the oracle consumes the device's bf16 h_{t-1} / DG_{t+1}, fp32 chains
run free.  bf16 outputs |got − ref| ≤ 2⁻⁸·|ref| + 2e-5·rms(ref), fp32-held outputs ≤ 2e-5·rms(ref).

Basis of the 2e-5 allowance at this file's longest reduction (backward, kC 5, C 40: 4000 terms): this oracle
free-running in torch fp32 on the host against itself in fp64 at C 40, kC 5, B 3, T 3, 9×17, worst tensor as a
fraction of rms(ref): forward (h, c, acts, tanh c) 2.1e-6, backward DG 6.9e-6, dc 2.3e-6, dh0 2.1e-6 — all under
1e-5, so the allowance stays at 2e-5.

Worst observed fraction of each bound on an MI355X: profiles/convlstm_errors.txt.
"""
import pytest
import torch
import torch.nn.functional as F

from test_rnn_oracle import NO, Draw, Guard, close_bf16, close_f32, d, dev, bf, f32, f64  # noqa: F401


# ------------------------------------------------------------------------------------------ the oracle
def conv(x, w):
    return F.conv2d(x, w, padding=w.shape[-1] // 2)


def dgrad(dg, Wh):
    """Σ_k DG_k ⊛ flip(Wh_k)ᵀ: the gradient of Σ_k conv(h, Wh_k) with respect to h."""
    C = Wh[0].shape[0]
    return sum(F.conv_transpose2d(dg[:, k * C:(k + 1) * C], Wh[k], padding=Wh[k].shape[-1] // 2) for k in range(4))


def _peep(peep, C, like):
    return (torch.zeros(3, 1, C, 1, 1, dtype=like.dtype) if peep is None else peep.reshape(3, 1, C, 1, 1))


def cell_fwd(gx, hp, cp, Wh, peep):
    """gx (B, 4C, H, W) input pre-activations, hp / cp (B, C, H, W), Wh four (C, C, k, k) → h, c, acts, tanh c."""
    C = hp.shape[1]
    pre = [gx[:, k * C:(k + 1) * C] + conv(hp, Wh[k]) for k in range(4)]
    p = _peep(peep, C, hp)
    i, f, g = torch.sigmoid(pre[0] + p[0] * cp), torch.sigmoid(pre[1] + p[1] * cp), torch.tanh(pre[3])
    c = f * cp + i * g
    o = torch.sigmoid(pre[2] + p[2] * c)
    tc = torch.tanh(c)
    return o * tc, c, torch.cat([i, f, o, g], 1), tc


def cell_bwd(dh, acts, tc, cp, dcn, peep):
    C = tc.shape[1]
    i, f, o, g = acts.split(C, 1)
    p = _peep(peep, C, tc)
    do = dh * tc * o * (1 - o)
    dc = dh * o * (1 - tc * tc) + dcn + do * p[2]
    di, df, dg = dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g)
    return torch.cat([di, df, do, dg], 1), dc * f + di * p[0] + df * p[1]


def seq_fwd(gx, h0, c0, Wh, peep, forced=None):
    """gx (T, B, 4C, H, W); ``forced`` (T+1, B, C, H, W): the hidden sequence whose slot t feeds step t."""
    h, c, outs = h0, c0, []
    for t in range(gx.shape[0]):
        h, c, a, tc = cell_fwd(gx[t], h if forced is None else forced[t], c, Wh, peep)
        outs.append((h, c, a, tc))
    return [torch.stack(v) for v in zip(*outs)]


def seq_bwd(gy, Wh, peep, acts, tcs, cs, c0, forced=None):
    T = gy.shape[0]
    DG, dc = [None] * T, torch.zeros_like(gy[0])
    for t in range(T - 1, -1, -1):
        dh = gy[t] + (dgrad(DG[t + 1] if forced is None else forced[t + 1], Wh) if t + 1 < T else 0)
        DG[t], dc = cell_bwd(dh, acts[t], tcs[t], cs[t - 1] if t else c0, dc, peep)
    return torch.stack(DG), dc


def peep_terms(DG, cs, c0):
    """(3, C, n) products whose sums over n are the peephole gradients."""
    C = cs.shape[2]
    cp = torch.cat([c0.unsqueeze(0), cs[:-1]])
    t = torch.stack([DG[:, :, :C] * cp, DG[:, :, C:2 * C] * cp, DG[:, :, 2 * C:3 * C] * cs])
    return t.permute(0, 3, 1, 2, 4, 5).reshape(3, C, -1)


def nhwc(t):
    return t.movedim(-3, -1).contiguous()


def nchw(t):
    return None if t is None else t.movedim(-1, -3)


def oihw(ws):
    return [d(w).permute(0, 3, 1, 2) for w in ws]


# ------------------------------------------------------------------------- CPU: the oracle is the layer
@pytest.mark.parametrize("with_peephole", (True, False))
def test_oracle_reproduces_fp64_layer(with_peephole):
    from bigdl.nn import ConvLSTMPeephole, Recurrent
    from bigdl.utils.table import T as Tbl
    B, T, Cin, C, H, W = 2, 3, 3, 4, 5, 6
    r = Draw(5, f64)
    x, gy = r.n(B, T, Cin, H, W), r.n(B, T, C, H, W)
    h0, c0 = r.h(B, C, H, W), r.n(B, C, H, W)
    rec = Recurrent().add(ConvLSTMPeephole(Cin, C, 3, 5, with_peephole=with_peephole)).to(dtype=f64)
    cell = rec.getCell()
    rec.training()
    rec.setHiddenState(Tbl(h0.clone(), c0.clone()))
    y = rec.forward(x)
    rec.zeroGradParameters()
    gi = rec.backward(x, gy)
    Wx = [m.weight.reshape(C, Cin, 3, 3) for m in cell.gx]
    Wh = [m.weight.reshape(C, C, 5, 5) for m in cell.gh]
    peep = torch.stack([m.weight.reshape(C) for m in cell.peep]) if with_peephole else None
    xt = x.transpose(0, 1)
    gx = torch.stack([torch.cat([conv(xt[t], w) + m.bias.view(1, C, 1, 1) for w, m in zip(Wx, cell.gx)], 1)
                      for t in range(T)])
    hs, cs, acts, tcs = seq_fwd(gx, h0, c0, Wh, peep)
    DG, gc = seq_bwd(gy.transpose(0, 1), Wh, peep, acts, tcs, cs, c0)
    hprev = torch.cat([h0.unsqueeze(0), hs[:-1]])
    figs = {"y": (y, hs.transpose(0, 1)), "gh": (rec.getGradHiddenState()[0], dgrad(DG[0], Wh)),
            "gc": (rec.getGradHiddenState()[1], gc),
            "gi": (gi, torch.stack([sum(F.conv_transpose2d(DG[t][:, k * C:(k + 1) * C], Wx[k], padding=1)
                                        for k in range(4)) for t in range(T)]).transpose(0, 1))}
    for k in range(4):
        dgk = DG[:, :, k * C:(k + 1) * C].reshape(T * B, C, H, W)
        figs[f"gWx{k}"] = (cell.gx[k].gradWeight.reshape(C, Cin, 3, 3),
                           torch.nn.grad.conv2d_weight(xt.reshape(T * B, Cin, H, W), (C, Cin, 3, 3), dgk, padding=1))
        figs[f"gWh{k}"] = (cell.gh[k].gradWeight.reshape(C, C, 5, 5),
                           torch.nn.grad.conv2d_weight(hprev.reshape(T * B, C, H, W), (C, C, 5, 5), dgk, padding=2))
        figs[f"gb{k}"] = (cell.gx[k].gradBias, dgk.sum((0, 2, 3)))
    if with_peephole:
        for k, m in enumerate(cell.peep):
            figs[f"gp{k}"] = (m.gradWeight.reshape(C), peep_terms(DG, cs, c0)[k].sum(1))
    for k, (a, b) in figs.items():
        v = float((a - b).abs().max())
        print(f"[convlstm] part=cpu what={k} maxdiff={v:.3e}")
        assert a.shape == b.shape and v <= 1e-12, (k, v)


# ---------------------------------------------------------------------------------- GPU: single steps
def _draw_weights(r, C, kC):
    return [r.n(C, kC, kC, C, scale=(kC * kC * C) ** -0.5) for _ in range(4)]  # [C_out][kC][kC][C_in]


def _step_case(NO, C, kC, H, W, B, null_c=False, null_dc=False, null_p=False):
    tag = f"C{C}:k{kC}:{H}x{W}:B{B}" + ":c=None" * null_c + ":dc=None" * null_dc + ":p=None" * null_p
    r, g = Draw(C * 1000 + kC * 100 + H * 10 + B), Guard()
    Wh = _draw_weights(r, C, kC)
    peep = None if null_p else r.n(3, C, scale=0.5, dt=f32)
    cp = None if null_c else r.n(B, H, W, C, dt=f32)
    zero = torch.zeros(B, C, H, W, dtype=f64)
    # forward
    hp, gx = r.h(B, H, W, C), r.n(B, H, W, 4 * C)
    h, c, act, tc = g.new((B, H, W, C), bf), g.new((B, H, W, C), f32), g.new((B, H, W, 4 * C), f32), g.new((B, H, W, C), f32)
    NO.convlstm_step("fwd", dev(hp), [dev(w) for w in Wh], B, H, W, C, kC, gx=dev(gx), c_prev=dev(cp), peep=dev(peep),
                     h_out=h, c_out=c, act=act, tc=tc)
    g.check()
    rh, rc, ra, rtc = cell_fwd(nchw(d(gx)), nchw(d(hp)), zero if null_c else nchw(d(cp)), oihw(Wh), d(peep))
    close_bf16("S", tag + ":h", h, nhwc(rh))
    close_f32("S", tag + ":c", c, nhwc(rc))
    for k, nm in enumerate("ifog"):
        close_f32("S", tag + ":act_" + nm, act[..., k * C:(k + 1) * C], nhwc(ra[:, k * C:(k + 1) * C]))
    close_f32("S", tag + ":tanh_c", tc, nhwc(rtc))
    # backward
    dgn, gy = r.n(B, H, W, 4 * C, scale=0.5), r.n(B, H, W, C)
    acts = torch.cat([r.sig(B, H, W, 3 * C), torch.tanh(r.n(B, H, W, C, dt=f32))], -1)
    tcv, dcn = torch.tanh(r.n(B, H, W, C, dt=f32)), None if null_dc else r.n(B, H, W, C, dt=f32)
    dg, dcp = g.new((B, H, W, 4 * C), bf), g.new((B, H, W, C), f32)
    wt = NO.convlstm_bwd_weights([dev(w) for w in Wh])
    NO.convlstm_step("bwd", dev(dgn), wt, B, H, W, C, kC, c_prev=dev(cp), peep=dev(peep), act=dev(acts), tc=dev(tcv),
                     gy=dev(gy), dc_next=dev(dcn), dg=dg, dc_prev=dcp)
    g.check()
    rdg, rdc = cell_bwd(nchw(d(gy)) + dgrad(nchw(d(dgn)), oihw(Wh)), nchw(d(acts)), nchw(d(tcv)),
                        zero if null_c else nchw(d(cp)), zero if null_dc else nchw(d(dcn)), d(peep))
    for k, nm in enumerate("ifog"):
        close_bf16("S", tag + ":dg_" + nm, dg[..., k * C:(k + 1) * C], nhwc(rdg[:, k * C:(k + 1) * C]))
    close_f32("S", tag + ":dc_prev", dcp, nhwc(rdc))


@pytest.mark.gpu
@pytest.mark.parametrize("HW", ((1, 1), (5, 7), (9, 17)))
@pytest.mark.parametrize("kC", (1, 3, 5))
@pytest.mark.parametrize("C", (8, 24, 40))
def test_steps(NO, C, kC, HW):
    for B in (1, 3):
        _step_case(NO, C, kC, *HW, B)


@pytest.mark.gpu
@pytest.mark.parametrize("null", ("null_c", "null_dc", "null_p"))
def test_steps_null_operands(NO, null):
    _step_case(NO, 24, 3, 5, 7, 3, **{null: True})


# ------------------------------------------------------------------------------------ GPU: sequences
@pytest.mark.gpu
@pytest.mark.parametrize("C", (8, 40))
@pytest.mark.parametrize("T", (1, 3))
def test_sequences(NO, T, C):
    B, H, W, kC = 3, 5, 7, 3
    tag, n = f"T{T}:C{C}", B * T * H * W
    r, g = Draw(77 * T + C), Guard()
    Wh, peep = _draw_weights(r, C, kC), r.n(3, C, scale=0.5, dt=f32)
    h0, c0, gx, gy = r.h(B, H, W, C), r.n(B, H, W, C, dt=f32), r.n(T, B, H, W, 4 * C), r.n(T, B, H, W, C)
    ws = [dev(w) for w in Wh]
    hs = g.new((T + 1, B, H, W, C), bf, init=torch.cat([h0.unsqueeze(0), torch.zeros(T, B, H, W, C, dtype=bf)]))
    cs, tcs, acts = g.new((T, B, H, W, C), f32), g.new((T, B, H, W, C), f32), g.new((T, B, H, W, 4 * C), f32)
    NO.convlstm_seq_forward(hs, dev(gx), dev(c0), ws, dev(peep), cs, acts, tcs, None)
    hs2, cbuf = hs.clone(), g.new((2, B, H, W, C), f32)
    hs2[1:].zero_()
    NO.convlstm_seq_forward(hs2, dev(gx), dev(c0), ws, dev(peep), None, None, None, cbuf)
    g.check()
    assert torch.equal(hs2, hs), tag + ": inference h differs from training h"
    assert torch.equal(cbuf[(T - 1) % 2], cs[T - 1]), tag
    rh, rc, ra, rtc = seq_fwd(nchw(d(gx)), None, nchw(d(c0)), oihw(Wh), d(peep), forced=nchw(d(hs)))
    close_bf16("Q", tag + ":h", hs[1:], nhwc(rh))
    for nm, got, ref in (("c", cs, rc), ("acts", acts, ra), ("tanh_c", tcs, rtc)):
        close_f32("Q", tag + ":" + nm, got, nhwc(ref))
    DG, gc, dh0 = g.new((T, B, H, W, 4 * C), bf), g.new((B, H, W, C), f32), g.new((B, H, W, C), f32)
    NO.convlstm_seq_backward(dev(gy), NO.convlstm_bwd_weights(ws), dev(peep), acts, tcs, cs, dev(c0), DG, gc, dh0)
    g.check()
    rdg, rgc = seq_bwd(nchw(d(gy)), oihw(Wh), d(peep), nchw(d(acts)), nchw(d(tcs)), nchw(d(cs)), nchw(d(c0)),
                       forced=nchw(d(DG)))
    close_bf16("Q", tag + ":DG", DG, nhwc(rdg))
    close_f32("Q", tag + ":gc", gc, nhwc(rgc))
    close_f32("Q", tag + ":dh0", dh0, nhwc(dgrad(nchw(d(DG[0])), oihw(Wh))))
    gp = [torch.zeros(3, C, device="cuda") for _ in range(2)]
    for t in gp:
        NO.convlstm_peephole_grad(DG, cs, dev(c0), t)
    assert torch.equal(gp[0], gp[1]), tag + ": peephole gradient not reproducible"
    terms = peep_terms(nchw(d(DG)), nchw(d(cs)), nchw(d(c0)))
    err, bound = (d(gp[0]) - terms.sum(2)).abs(), n * 2.0 ** -24 * terms.abs().sum(2)
    print(f"[rnn-oracle] part=Q what={tag}:gp frac={float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), tag


# ---------------------------------------------------------------------------------------- GPU: layer
def _gpu_layer(cell_fn):
    import bigdl.nn as nn
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    torch.manual_seed(0)
    ref = nn.Recurrent().add(cell_fn(nn))
    return ref, ref.cloneModule().to(device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("with_peephole", (True, False))
def test_layer_native_vs_fp64(with_peephole):
    from bigdl import ops
    from bigdl.utils import config
    ref, gpu = _gpu_layer(lambda nn: nn.ConvLSTMPeephole(16, 24, 3, 3, with_peephole=with_peephole))
    x, gy = torch.randn(3, 3, 16, 9, 17), torch.randn(3, 3, 24, 9, 17)
    ops.reset_fallbacks()
    res = []
    for m, cv in ((ref.to(dtype=f64), torch.Tensor.double), (gpu, torch.Tensor.cuda)):
        m.training()
        y, tag = m.forward(cv(x)), m._rec[0]
        m.zeroGradParameters()
        res.append([y, m.backward(cv(x), cv(gy))] + m.parameters()[1])
    assert tag == "convlstm", tag
    assert ops.fallback_counts() == {}, ops.fallback_counts()
    for k, (b, a) in enumerate(zip(*res)):
        torch.testing.assert_close(a.double().cpu(), b, rtol=5e-2, atol=5e-2 * (float(b.abs().max()) if k >= 2 else 1.0))
    try:
        config.set_property("bigdl.rnn.nativeConvLSTM", False)
        gpu.forward(x.cuda())
        assert gpu._rec[0] == "generic", gpu._rec[0]
    finally:
        config.set_property("bigdl.rnn.nativeConvLSTM", True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("stride2", "activation"))
def test_ineligible_cells_stay_generic(kind):
    _, gpu = _gpu_layer(lambda nn: nn.ConvLSTMPeephole(16, 24, 3, 3, stride=2) if kind == "stride2"
                        else nn.ConvLSTMPeephole(16, 24, 3, 3, activation=nn.Sigmoid()))
    gpu.training()
    hw = 1 if kind == "stride2" else 8  # a strided cell keeps its hidden shape only on 1×1 images
    gpu.forward(torch.randn(2, 2, 16, hw, hw).cuda())
    assert gpu._rec[0] == "generic", gpu._rec[0]
