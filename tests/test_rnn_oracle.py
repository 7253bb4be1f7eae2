"""The fused recurrent step kernels (rnn_step.hip: k_rnn_step<CELL, G>, k_rnn_step_pair, their bf16x3
fp32 forms) and the whole-sequence launchers built on them, against a plain torch fp64 evaluation of
the same steps on the host.

Oracle.  Written from the reference's equations, not from the kernel: ``DL/nn/LSTM.scala:124-187``
(gates i, g, f, o; c = i·g + f·c₋₁; h = o·tanh c), ``DL/nn/GRU.scala`` (r, z = σ(x_rz + h U_rzᵀ);
n = tanh(x_h + (r∘h) U_hᵀ); h′ = (1−z)n + z h) and the BPTT of ``DL/nn/Recurrent.scala:283-400``.  The
unmarked test at the top runs it free (no forcing, no rounding) against ``Recurrent().add(LSTM)`` and
``Recurrent().add(GRU)`` converted to float64 with a non-zero ``setHiddenState``: output, input gradient
through the pre-topology, ``getGradHiddenState()`` and the recurrent ``gradWeight`` agree within 1e-12
(observed 0.0 for the LSTM and ≤ 4.5e-16 for the GRU at B 3, T 3, IN 5, H 8).

Teacher forcing.  Inputs are drawn in fp32 and rounded once to the kernel's operand type; weights are
N(0, 1/K) so pre-activations are O(1); h0 = tanh(randn), c0 = randn (never zero, one extra case passes
``c0 = None``).  Every bf16-rounded quantity that a later step consumes is fed to the oracle as the kernel
wrote it (``out[:, t−1]``, the GRU's ``RH[:, t]``, layer 0's ``out0[:, t]`` for layer 1 of the pair;
``DG[:, t+1]``, the GRU's ``DG[:, t, 2H:]``, ``DG1[:, t]`` for layer 0 of the pair); every fp32-held
quantity (c, dc, the GRU carry, the fp32 saves) runs free in fp64.  Each step is therefore one bf16
rounding away from fp64 whatever T is, and a wrong step shows at that step.

Guard bands.  Every output tensor is a 16-byte-aligned contiguous slice of a larger buffer pre-filled
with the byte 0x7F (bf16 / fp32 3.39e38: an element the kernel skips cannot pass either); the bytes
outside the slice must be untouched after the call.

Bounds (none taken from the code under test):
  bf16 outputs (h, rh, dg)   per element |got − ref| ≤ 2⁻⁸·|ref| + 2e-5·rms(ref).  2⁻⁸ is the bf16 unit
                             roundoff; the absolute term is the fp32-accumulation allowance of
                             tests/test_bf16_kernel_variants.py: the kernel rounds an fp32 value that is
                             itself that far from fp64.  The bf16-rounded reference alone reaches
                             0.86–0.99 of the relative term, so the coefficient cannot be smaller.
  fp32-held outputs          |got − ref| ≤ 2e-5·rms(ref)   (cs, acts, tcs, gc, R, Z, Nn, carry)
  part F (bf16x3 products)   |got − ref| ≤ 1e-4·max|ref| per tensor, the bound tests/test_rnn_fp32.py
                             holds that path to.
Basis of the 2e-5 allowance: this module's oracle evaluated in torch fp32 on the host against itself in
fp64, free-running at the widest shape (H 264, B 33, T 3), worst tensor as a fraction of rms(ref):
  LSTM forward  (out, cs, acts, tcs)      1.0e-6
  LSTM backward (DG, gc: 3-step dc chain) 3.7e-6
  GRU forward   (out, R, Z, Nn, RH)       1.1e-6
  GRU backward  (DG, 3-step carry chain)  1.5e-6
all far under half the allowance (1e-5), so it stays at 2e-5.

Worst observed fraction of each bound per part on an MI355X (profiles/rnn_oracle_errors.txt), bf16 / fp32:
  S 0.991 / 0.025, L 0.991 / 0.066, G 0.992 / 0.050, P 0.992 / 0.094, F 0.101 of 1e-4·max; Li, Gi bit-equal.

Shapes.  Per-step path only (``BIGDL_RNN_PERSIST=0``); T ∈ {1, 3}: T = 1 makes the first step also the
last (the ``t == 0`` operand has row stride H, not T·H), T = 3 takes both ``lda`` forms and both parities
of the inference ``cbuf`` ping-pong.  H ∈ {8, 24, 40, 264} × M ∈ {1, 16, 17, 33}: a partial-only unit
tile, full + partial, 17 tiles; one half tile, an exact half, a half plus one row, a second batch block;
K = 8 (only lanes fq = 0 live), 24 / 40 (a partly filled 32-chunk), 264 forward and 1056 backward (waves
take a second chunk, the last chunk holds 8 columns).  The pair (H0, H1) ∈ {(24, 40), (40, 8), (264, 24)}
puts the forward segment boundary at K = 40 / 8 / 24 inside a 32-chunk, the backward one at 4·H0, sizes
the grid by either layer, and runs the ``live`` mask at w = 0 and w = T with b1 ≠ 0.
"""
import math

import pytest
import torch

bf = torch.bfloat16
f32 = torch.float32
f64 = torch.float64

U_BF16 = 2.0 ** -8     # bf16 unit roundoff
ABS = 2e-5             # fp32-accumulation allowance, × rms(ref)
TOL_X3 = 1e-4          # bf16x3 path, × max|ref|
SENT, PAD = 0x7F, 256  # guard byte and guard-band width (bytes)

SHAPES_H = (8, 24, 40, 264)
SHAPES_M = (1, 16, 17, 33)
TS = (1, 3)


# ------------------------------------------------------------------------------------------ the oracle
def lstm_cell_fwd(pre, c_prev):
    """pre [M][4H] gate pre-activations (i, g, f, o) → h, c, acts [M][4H], tanh c."""
    H = pre.shape[1] // 4
    i, g = torch.sigmoid(pre[:, :H]), torch.tanh(pre[:, H:2 * H])
    f, o = torch.sigmoid(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
    c = i * g + f * c_prev
    tc = torch.tanh(c)
    return o * tc, c, torch.cat([i, g, f, o], 1), tc


def lstm_cell_bwd(dh, acts, tc, c_prev, dc_next):
    """Gradient of :func:`lstm_cell_fwd`: dh, dc_next → gate-pre-activation gradients [M][4H], dc₋₁."""
    H = tc.shape[1]
    i, g, f, o = acts[:, :H], acts[:, H:2 * H], acts[:, 2 * H:3 * H], acts[:, 3 * H:]
    dc = dh * o * (1 - tc * tc) + dc_next
    do = dh * tc
    dg = torch.cat([dc * g * i * (1 - i), dc * i * (1 - g * g), dc * c_prev * f * (1 - f), do * o * (1 - o)], 1)
    return dg, dc * f


def lstm_fwd(x2, h0, c0, U, forced=None):
    """x2 [B][T][4H] input projection, U [4H][H] → out [B][T][H], cs, acts, tcs [T][B][·].
    ``forced``: the hidden sequence whose step t−1 feeds step t (the device's bf16 out) instead of the
    oracle's own."""
    B, T, _ = x2.shape
    c = torch.zeros_like(h0) if c0 is None else c0
    out, cs, acts, tcs = [], [], [], []
    for t in range(T):
        hp = h0 if t == 0 else (forced[:, t - 1] if forced is not None else out[-1])
        h, c, a, tc = lstm_cell_fwd(x2[:, t] + hp @ U.t(), c)
        out.append(h), cs.append(c), acts.append(a), tcs.append(tc)
    return torch.stack(out, 1), torch.stack(cs), torch.stack(acts), torch.stack(tcs)


def lstm_bwd(gy, U, acts, tcs, cs, c0, forced=None):
    """BPTT: dh_t = gy_t + dg_{t+1}·U → DG [B][T][4H], dc before the first step.  ``forced``: the gate
    gradients whose step t+1 feeds step t (the device's bf16 DG)."""
    B, T, H = gy.shape
    DG = [None] * T
    dc = torch.zeros_like(gy[:, 0])
    for t in range(T - 1, -1, -1):
        dh = gy[:, t]
        if t + 1 < T:
            dh = dh + (forced[:, t + 1] if forced is not None else DG[t + 1]) @ U
        c_prev = cs[t - 1] if t > 0 else (torch.zeros_like(dc) if c0 is None else c0)
        DG[t], dc = lstm_cell_bwd(dh, acts[t], tcs[t], c_prev, dc)
    return torch.stack(DG, 1), dc


def gru_rz(pre, h_prev):
    H = h_prev.shape[1]
    r, z = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:])
    return r, z, r * h_prev


def gru_n(pre, z, h_prev):
    n = torch.tanh(pre)
    return n, (1 - z) * n + z * h_prev


def gru_bwd_zn(dh, z, n, h_prev):
    """h′ = (1−z)n + z h: dh′ → da_z, da_n and the direct part dh′·z of dh."""
    return dh * (h_prev - n) * z * (1 - z), dh * (1 - z) * (1 - n * n), dh * z


def gru_bwd_r(drh, r, h_prev):
    """rh = r∘h: d(rh) → da_r and the part d(rh)·r of dh."""
    return drh * h_prev * r * (1 - r), drh * r


def gru_fwd(x2, h0, Urz, Uh, forced=None, forced_rh=None):
    """x2 [B][T][3H] (r, z, h blocks), U_rz [2H][H], U_h [H][H] → out, RH [B][T][H]; R, Z, Nn [T][B][H]."""
    B, T, _ = x2.shape
    H = h0.shape[1]
    out, R, Z, Nn, RH = [], [], [], [], []
    for t in range(T):
        hp = h0 if t == 0 else (forced[:, t - 1] if forced is not None else out[-1])
        r, z, rh = gru_rz(x2[:, t, :2 * H] + hp @ Urz.t(), hp)
        rh_in = forced_rh[:, t] if forced_rh is not None else rh
        n, h = gru_n(x2[:, t, 2 * H:] + rh_in @ Uh.t(), z, hp)
        out.append(h), R.append(r), Z.append(z), Nn.append(n), RH.append(rh)
    return torch.stack(out, 1), torch.stack(R), torch.stack(Z), torch.stack(Nn), torch.stack(RH, 1)


def gru_bwd(gy, Urz, Uh, R, Z, Nn, hprev, carry, forced=None):
    """hprev [B][T][H] = (h0, out[:, :-1]); carry = dh arriving from beyond the last step.  Returns
    DG [B][T][3H] (da_r, da_z, da_n) and the carry before the first step (dh0 without da_rz_0·U_rz)."""
    B, T, H = gy.shape
    DG = [None] * T
    for t in range(T - 1, -1, -1):
        dh = gy[:, t] + carry
        if t + 1 < T:
            dh = dh + (forced[:, t + 1, :2 * H] if forced is not None else DG[t + 1][:, :2 * H]) @ Urz
        da_z, da_n, carry = gru_bwd_zn(dh, Z[t], Nn[t], hprev[:, t])
        drh = (forced[:, t, 2 * H:] if forced is not None else da_n) @ Uh
        da_r, more = gru_bwd_r(drh, R[t], hprev[:, t])
        carry = carry + more
        DG[t] = torch.cat([da_r, da_z, da_n], 1)
    return torch.stack(DG, 1), carry


def _hprev(h0, out):
    return torch.cat([h0.unsqueeze(1), out[:, :-1]], 1)


# ------------------------------------------------------------------------- CPU self-check of the oracle
def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


def test_oracle_reproduces_fp64_recurrent_layers():
    """The oracle, free-running and unrounded, is the fp64 CPU ``Recurrent`` of LSTM and GRU."""
    from bigdl.nn import GRU, LSTM, Recurrent
    from bigdl.utils.table import T as Tbl
    B, T, IN, H = 3, 3, 5, 8
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, IN, generator=g, dtype=f64)
    gy = torch.randn(B, T, H, generator=g, dtype=f64)
    h0 = torch.tanh(torch.randn(B, H, generator=g, dtype=f64))
    c0 = torch.randn(B, H, generator=g, dtype=f64)

    rec = Recurrent().add(LSTM(IN, H)).to(dtype=f64)
    rec.training()
    rec.setHiddenState(Tbl(h0.clone(), c0.clone()))
    y = rec.forward(x)
    rec.zeroGradParameters()
    gi = rec.backward(x, gy)
    (Wi, bi, U), (_, _, gU) = rec.parameters()
    out, cs, acts, tcs = lstm_fwd(x @ Wi.t() + bi, h0, c0, U)
    DG, gc = lstm_bwd(gy, U, acts, tcs, cs, c0)
    gh = rec.getGradHiddenState()
    figs = {"lstm:y": _maxdiff(y, out), "lstm:gi": _maxdiff(gi, DG @ Wi), "lstm:gh": _maxdiff(gh[0], DG[:, 0] @ U),
            "lstm:gc": _maxdiff(gh[1], gc),
            "lstm:gU": _maxdiff(gU, torch.einsum("btg,bth->gh", DG, _hprev(h0, out)))}

    rec = Recurrent().add(GRU(IN, H)).to(dtype=f64)
    rec.training()
    rec.setHiddenState(h0.clone())
    y = rec.forward(x)
    rec.zeroGradParameters()
    gi = rec.backward(x, gy)
    (Wi, bi, Urz, Uh), (_, _, gUrz, gUh) = rec.parameters()
    out, R, Z, Nn, RH = gru_fwd(x @ Wi.t() + bi, h0, Urz, Uh)
    DG, carry = gru_bwd(gy, Urz, Uh, R, Z, Nn, _hprev(h0, out), torch.zeros_like(h0))
    figs.update({"gru:y": _maxdiff(y, out), "gru:gi": _maxdiff(gi, DG @ Wi),
                 "gru:gh": _maxdiff(rec.getGradHiddenState()[0], carry + DG[:, 0, :2 * H] @ Urz),
                 "gru:gUrz": _maxdiff(gUrz, torch.einsum("btg,bth->gh", DG[:, :, :2 * H], _hprev(h0, out))),
                 "gru:gUh": _maxdiff(gUh, torch.einsum("btg,bth->gh", DG[:, :, 2 * H:], RH))})
    for k, v in figs.items():
        print(f"[rnn-oracle] part=cpu what={k} maxdiff={v:.3e}")
    for k, v in figs.items():
        assert v <= 1e-12, (k, v)


# --------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture
def NO(monkeypatch):
    """native_ops on the per-step path, with the no-fallback check of tests/test_native_gemm_rnn.py."""
    from bigdl import ops
    from bigdl.ops import native_ops
    monkeypatch.setenv("BIGDL_RNN_PERSIST", "0")
    st = ops.native_status()
    assert st["loaded"], st
    ops.reset_fallbacks()
    yield native_ops
    assert ops.fallback_counts() == {}, ops.fallback_counts()


class Guard:
    """Output tensors as aligned slices of sentinel-filled buffers; ``check`` proves the bands intact."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype, init=None):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((PAD + n + PAD,), SENT, dtype=torch.uint8, device="cuda")
        self.bufs.append((buf, n))
        t = buf[PAD:PAD + n].view(dtype).view(*shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        if init is not None:
            t.copy_(init)
        return t

    def check(self):
        torch.cuda.synchronize()
        for k, (buf, n) in enumerate(self.bufs):
            assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), f"guard band {k} written"


def _report(part, what, frac):
    """One figure (fraction of its bound), printed before it is asserted (pytest -s / -rP collects the lines)."""
    print(f"[rnn-oracle] part={part} what={what} frac={frac:.3e}")
    assert frac <= 1.0, (part, what, frac)


def _rms(ref):
    return float(ref.pow(2).mean().sqrt())


def close_bf16(part, what, got, ref):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if _rms(ref) == 0:  # an identically zero reference (df with c₋₁ = None) must come out exactly zero
        return _report(part, what, 0.0 if not got.any() else math.inf)
    _report(part, what, float(((got - ref).abs() / (U_BF16 * ref.abs() + ABS * _rms(ref))).max()))


def close_f32(part, what, got, ref):
    got, ref = got.double().cpu(), ref.double()
    assert got.dtype == f64 and got.shape == ref.shape, (what, got.shape, ref.shape)
    _report(part, what, float((got - ref).abs().max()) / (ABS * _rms(ref)))


def close_x3(part, what, got, ref):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    _report(part, what, float((got - ref).abs().max()) / (TOL_X3 * float(ref.abs().max())))


class Draw:
    """Inputs drawn in fp32 on the host and rounded once to the operand type ``dt``."""

    def __init__(self, seed, dt=bf):
        self.g = torch.Generator().manual_seed(seed)
        self.dt = dt

    def n(self, *shape, scale=1.0, dt=None):
        return (torch.randn(*shape, generator=self.g) * scale).to(dt or self.dt)

    def w(self, rows, K):
        return self.n(rows, K, scale=K ** -0.5)

    def h(self, *shape):
        return torch.tanh(torch.randn(*shape, generator=self.g)).to(self.dt)

    def sig(self, *shape):
        return torch.sigmoid(torch.randn(*shape, generator=self.g))


def dev(t):
    return None if t is None else t.cuda()


def d(t):
    return None if t is None else t.double().cpu()


def tr(w):
    """Transposed weight as the backward kernels take it (exact)."""
    return w.t().contiguous()


# -------------------------------------------------------------------------- part S: one step per cell
def _step_case(NO, cell, H, M, null_c=False):
    part = "S"
    tag = f"cell{cell}:H{H}:M{M}" + (":c0=None" if null_c else "")
    r = Draw(1000 * cell + 10 * H + M)
    g = Guard()
    hp = r.h(M, H)
    if cell == 0:
        xg, U, c_prev = r.n(M, 4 * H), r.w(4 * H, H), None if null_c else r.n(M, H, dt=f32)
        h, c, act, tc = g.new((M, H), bf), g.new((M, H), f32), g.new((M, 4 * H), f32), g.new((M, H), f32)
        NO.rnn_step("lstm_fwd", dev(hp), dev(U), M, H, H, xg=dev(xg), c_prev=dev(c_prev), h_out=h, c_out=c, act=act,
                    tc=tc)
        g.check()
        rh_, rc, ra, rtc = lstm_cell_fwd(d(xg) + d(hp) @ d(U).t(), 0 if null_c else d(c_prev))
        close_bf16(part, tag + ":h", h, rh_)
        close_f32(part, tag + ":c", c, rc)
        for k, nm in enumerate("igfo"):
            close_f32(part, tag + ":act_" + nm, act[:, k * H:(k + 1) * H], ra[:, k * H:(k + 1) * H])
        close_f32(part, tag + ":tanh_c", tc, rtc)
    elif cell == 1:
        dgn, Ut, gy = r.n(M, 4 * H, scale=0.5), r.w(H, 4 * H), r.n(M, H)
        act = torch.cat([r.sig(M, H), torch.tanh(r.n(M, H, dt=f32)), r.sig(M, H), r.sig(M, H)], 1)
        tc, c_prev, gcn = torch.tanh(r.n(M, H, dt=f32)), None if null_c else r.n(M, H, dt=f32), r.n(M, H, dt=f32)
        dg, dcp = g.new((M, 4 * H), bf), g.new((M, H), f32)
        NO.rnn_step("lstm_bwd", dev(dgn), dev(Ut), M, 4 * H, H, c_prev=dev(c_prev), act=dev(act), tc=dev(tc),
                    gy=dev(gy), gc_next=dev(gcn), dg=dg, dc_prev=dcp)
        g.check()
        rdg, rdc = lstm_cell_bwd(d(gy) + d(dgn) @ d(Ut).t(), d(act), d(tc), 0 if null_c else d(c_prev), d(gcn))
        for k, nm in enumerate("igfo"):
            close_bf16(part, tag + ":dg_" + nm, dg[:, k * H:(k + 1) * H], rdg[:, k * H:(k + 1) * H])
        close_f32(part, tag + ":dc_prev", dcp, rdc)
    elif cell == 2:
        xg, Urz = r.n(M, 3 * H), r.w(2 * H, H)
        rh, R, Z = g.new((M, H), bf), g.new((M, H), f32), g.new((M, H), f32)
        NO.rnn_step("gru_fwd1", dev(hp), dev(Urz), M, H, H, xg=dev(xg), hprev=dev(hp), s0=R, s1=Z, rh=rh)
        g.check()
        rr, rz, rrh = gru_rz(d(xg)[:, :2 * H] + d(hp) @ d(Urz).t(), d(hp))
        close_f32(part, tag + ":r", R, rr)
        close_f32(part, tag + ":z", Z, rz)
        close_bf16(part, tag + ":rh", rh, rrh)
    elif cell == 3:
        xg, Uh, rh, z = r.n(M, 3 * H), r.w(H, H), r.h(M, H), r.sig(M, H)
        h, Nn = g.new((M, H), bf), g.new((M, H), f32)
        NO.rnn_step("gru_fwd2", dev(rh), dev(Uh), M, H, H, xg=dev(xg), hprev=dev(hp), h_out=h, s1=dev(z), s2=Nn)
        g.check()
        rn, rh_ = gru_n(d(xg)[:, 2 * H:] + d(rh) @ d(Uh).t(), d(z), d(hp))
        close_f32(part, tag + ":n", Nn, rn)
        close_bf16(part, tag + ":h", h, rh_)
    elif cell == 4:
        darz, Urz_t, gy = r.n(M, 2 * H, scale=0.5), r.w(H, 2 * H), r.n(M, H)
        c_in, z, n = r.n(M, H, dt=f32), r.sig(M, H), torch.tanh(r.n(M, H, dt=f32))
        dg, carry = g.new((M, 3 * H), bf), g.new((M, H), f32, init=c_in)
        NO.rnn_step("gru_bwd1", dev(darz), dev(Urz_t), M, 2 * H, H, hprev=dev(hp), gy=dev(gy), dg=dg, s0=carry,
                    s1=dev(z), s2=dev(n))
        g.check()
        rz, rn, rc = gru_bwd_zn(d(gy) + d(c_in) + d(darz) @ d(Urz_t).t(), d(z), d(n), d(hp))
        close_bf16(part, tag + ":da_z", dg[:, H:2 * H], rz)
        close_bf16(part, tag + ":da_n", dg[:, 2 * H:], rn)
        close_f32(part, tag + ":carry", carry, rc)
        assert bool((dg[:, :H].contiguous().view(torch.uint8) == SENT).all()), tag + ": da_r slot written by cell 4"
    else:
        dan, Uh_t, c_in, rr = r.n(M, H, scale=0.5), r.w(H, H), r.n(M, H, dt=f32), r.sig(M, H)
        dg, carry = g.new((M, 3 * H), bf), g.new((M, H), f32, init=c_in)
        NO.rnn_step("gru_bwd2", dev(dan), dev(Uh_t), M, H, H, hprev=dev(hp), dg=dg, s0=carry, s1=dev(rr))
        g.check()
        rda, more = gru_bwd_r(d(dan) @ d(Uh_t).t(), d(rr), d(hp))
        close_bf16(part, tag + ":da_r", dg[:, :H], rda)
        close_f32(part, tag + ":carry", carry, d(c_in) + more)
        assert bool((dg[:, H:].contiguous().view(torch.uint8) == SENT).all()), tag + ": z/n slots written by cell 5"


@pytest.mark.gpu
@pytest.mark.parametrize("H", SHAPES_H)
@pytest.mark.parametrize("cell", range(6))
def test_step_cells(NO, cell, H):
    for M in SHAPES_M:
        _step_case(NO, cell, H, M)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [0, 1])
def test_step_null_c_prev(NO, cell):
    _step_case(NO, cell, 24, 17, null_c=True)


# ------------------------------------------------------------ parts L / Li / F: single-layer LSTM sequence
def _lstm_inputs(r, B, T, H, null_c=False):
    dt32 = f32
    return dict(x2=r.n(B, T, 4 * H), h0=r.h(B, H), c0=None if null_c else r.n(B, H, dt=dt32), U=r.w(4 * H, H),
                gy=r.n(B, T, H))


def _lstm_train_fwd(NO, g, v, fwd):
    B, T, G = v["x2"].shape
    H = G // 4
    dt = v["x2"].dtype
    o = dict(out=g.new((B, T, H), dt), cs=g.new((T, B, H), f32), acts=g.new((T, B, 4 * H), f32),
             tcs=g.new((T, B, H), f32))
    fwd(dev(v["x2"]), dev(v["h0"]), dev(v["c0"]), dev(v["U"]), o["out"], o["cs"], o["acts"], o["tcs"], None)
    return o


def _lstm_case(NO, B, T, H, null_c=False):
    part = "L"
    tag = f"H{H}:B{B}:T{T}" + (":c0=None" if null_c else "")
    v = _lstm_inputs(Draw(7000 + 100 * H + 4 * B + T), B, T, H, null_c)
    g = Guard()
    o = _lstm_train_fwd(NO, g, v, NO.lstm_seq_forward)
    DG, gc = g.new((B, T, 4 * H), bf), g.new((B, H), f32)
    NO.lstm_seq_backward(dev(v["gy"]), dev(tr(v["U"])), o["acts"], o["tcs"], o["cs"], dev(v["c0"]), DG, gc)
    g.check()
    U = d(v["U"])
    out, cs, acts, tcs = lstm_fwd(d(v["x2"]), d(v["h0"]), d(v["c0"]), U, forced=d(o["out"]))
    rDG, rgc = lstm_bwd(d(v["gy"]), U, acts, tcs, cs, d(v["c0"]), forced=d(DG))
    for t in range(T):
        close_bf16(part, f"{tag}:out[{t}]", o["out"][:, t], out[:, t])
        close_f32(part, f"{tag}:cs[{t}]", o["cs"][t], cs[t])
        for k, nm in enumerate("igfo"):
            close_f32(part, f"{tag}:acts_{nm}[{t}]", o["acts"][t][:, k * H:(k + 1) * H], acts[t][:, k * H:(k + 1) * H])
        close_f32(part, f"{tag}:tcs[{t}]", o["tcs"][t], tcs[t])
        for k, nm in enumerate("igfo"):
            close_bf16(part, f"{tag}:DG_{nm}[{t}]", DG[:, t, k * H:(k + 1) * H], rDG[:, t, k * H:(k + 1) * H])
    close_f32(part, f"{tag}:gc", gc, rgc)


@pytest.mark.gpu
@pytest.mark.parametrize("B", SHAPES_M)
@pytest.mark.parametrize("H", SHAPES_H)
def test_lstm_sequence(NO, H, B):
    for T in TS:
        _lstm_case(NO, B, T, H)


@pytest.mark.gpu
def test_lstm_sequence_null_c0(NO):
    _lstm_case(NO, 17, 3, 24, null_c=True)


INFER = [(24, 17, 3), (264, 33, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,B,T", INFER)
def test_lstm_inference_bit_equal(NO, H, B, T):
    v = _lstm_inputs(Draw(8000 + H + B + T), B, T, H)
    g = Guard()
    o = _lstm_train_fwd(NO, g, v, NO.lstm_seq_forward)
    out, cbuf = g.new((B, T, H), bf), g.new((2, B, H), f32)
    NO.lstm_seq_forward(dev(v["x2"]), dev(v["h0"]), dev(v["c0"]), dev(v["U"]), out, None, None, None, cbuf)
    g.check()
    assert torch.equal(out.view(torch.int16), o["out"].view(torch.int16)), "Li: out"
    assert torch.equal(cbuf[(T - 1) % 2].view(torch.int32), o["cs"][T - 1].view(torch.int32)), "Li: cbuf"
    print(f"[rnn-oracle] part=Li what=H{H}:B{B}:T{T} frac=0.000e+00")


F_H, F_B = (8, 40, 264), (1, 17, 33)


@pytest.mark.gpu
@pytest.mark.parametrize("B", F_B)
@pytest.mark.parametrize("H", F_H)
def test_lstm_sequence_fp32(NO, H, B):
    """bf16x3 recurrent products, free-running against the free-running oracle."""
    part, T, tag = "F", 3, f"lstm:H{H}:B{B}"
    v = _lstm_inputs(Draw(9000 + 10 * H + B, dt=f32), B, T, H)
    g = Guard()
    o = _lstm_train_fwd(NO, g, v, NO.lstm_seq_forward32)
    DG, gc = g.new((B, T, 4 * H), f32), g.new((B, H), f32)
    NO.lstm_seq_backward32(dev(v["gy"]), dev(tr(v["U"])), o["acts"], o["tcs"], o["cs"], dev(v["c0"]), DG, gc)
    g.check()
    U = d(v["U"])
    out, cs, acts, tcs = lstm_fwd(d(v["x2"]), d(v["h0"]), d(v["c0"]), U)
    rDG, rgc = lstm_bwd(d(v["gy"]), U, acts, tcs, cs, d(v["c0"]))
    for nm, got, ref in (("out", o["out"], out), ("cs", o["cs"], cs), ("acts", o["acts"], acts),
                         ("tcs", o["tcs"], tcs), ("DG", DG, rDG), ("gc", gc, rgc)):
        close_x3(part, f"{tag}:{nm}", got, ref)


# ------------------------------------------------------------------ parts G / Gi / F: GRU sequence
def _gru_inputs(r, B, T, H):
    return dict(x2=r.n(B, T, 3 * H), h0=r.h(B, H), Urz=r.w(2 * H, H), Uh=r.w(H, H), gy=r.n(B, T, H),
                carry=r.n(B, H, dt=f32))


def _gru_run(NO, g, v, fwd, bwd):
    B, T, G = v["x2"].shape
    H = G // 3
    dt = v["x2"].dtype
    o = dict(out=g.new((B, T, H), dt), R=g.new((T, B, H), f32), Z=g.new((T, B, H), f32), Nn=g.new((T, B, H), f32),
             RH=g.new((B, T, H), dt), DG=g.new((B, T, 3 * H), dt), carry=g.new((B, H), f32, init=v["carry"]))
    h0 = dev(v["h0"])
    fwd(dev(v["x2"]), h0, dev(v["Urz"]), dev(v["Uh"]), o["out"], o["R"], o["Z"], o["Nn"], o["RH"], True)
    bwd(dev(v["gy"]), dev(tr(v["Urz"])), dev(tr(v["Uh"])), o["R"], o["Z"], o["Nn"], o["out"], h0, o["DG"], o["carry"])
    g.check()
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("B", SHAPES_M)
@pytest.mark.parametrize("H", SHAPES_H)
def test_gru_sequence(NO, H, B):
    part = "G"
    for T in TS:
        tag = f"H{H}:B{B}:T{T}"
        v = _gru_inputs(Draw(17000 + 100 * H + 4 * B + T), B, T, H)
        o = _gru_run(NO, Guard(), v, NO.gru_seq_forward, NO.gru_seq_backward)
        Urz, Uh, h0 = d(v["Urz"]), d(v["Uh"]), d(v["h0"])
        out, R, Z, Nn, RH = gru_fwd(d(v["x2"]), h0, Urz, Uh, forced=d(o["out"]), forced_rh=d(o["RH"]))
        rDG, rcarry = gru_bwd(d(v["gy"]), Urz, Uh, R, Z, Nn, _hprev(h0, d(o["out"])), d(v["carry"]),
                              forced=d(o["DG"]))
        for t in range(T):
            close_bf16(part, f"{tag}:out[{t}]", o["out"][:, t], out[:, t])
            close_bf16(part, f"{tag}:RH[{t}]", o["RH"][:, t], RH[:, t])
            for nm, ref in (("R", R), ("Z", Z), ("Nn", Nn)):
                close_f32(part, f"{tag}:{nm}[{t}]", o[nm][t], ref[t])
            for k, nm in enumerate(("da_r", "da_z", "da_n")):
                close_bf16(part, f"{tag}:{nm}[{t}]", o["DG"][:, t, k * H:(k + 1) * H], rDG[:, t, k * H:(k + 1) * H])
        close_f32(part, f"{tag}:carry", o["carry"], rcarry)


@pytest.mark.gpu
@pytest.mark.parametrize("H,B,T", INFER)
def test_gru_inference_bit_equal(NO, H, B, T):
    v = _gru_inputs(Draw(18000 + H + B + T), B, T, H)
    g = Guard()
    args = [dev(v[k]) for k in ("x2", "h0", "Urz", "Uh")]
    ref = g.new((B, T, H), bf)
    NO.gru_seq_forward(*args, ref, g.new((T, B, H), f32), g.new((T, B, H), f32), g.new((T, B, H), f32),
                       g.new((B, T, H), bf), True)
    out = g.new((B, T, H), bf)
    NO.gru_seq_forward(*args, out, g.new((1, B, H), f32), g.new((1, B, H), f32), None, g.new((B, 1, H), bf), False)
    g.check()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "Gi: out"
    print(f"[rnn-oracle] part=Gi what=H{H}:B{B}:T{T} frac=0.000e+00")


@pytest.mark.gpu
@pytest.mark.parametrize("B", F_B)
@pytest.mark.parametrize("H", F_H)
def test_gru_sequence_fp32(NO, H, B):
    part, T, tag = "F", 3, f"gru:H{H}:B{B}"
    v = _gru_inputs(Draw(19000 + 10 * H + B, dt=f32), B, T, H)
    o = _gru_run(NO, Guard(), v, NO.gru_seq_forward32, NO.gru_seq_backward32)
    Urz, Uh, h0 = d(v["Urz"]), d(v["Uh"]), d(v["h0"])
    out, R, Z, Nn, RH = gru_fwd(d(v["x2"]), h0, Urz, Uh)
    rDG, rcarry = gru_bwd(d(v["gy"]), Urz, Uh, R, Z, Nn, _hprev(h0, out), d(v["carry"]))
    for nm, ref in (("out", out), ("R", R), ("Z", Z), ("Nn", Nn), ("RH", RH), ("DG", rDG), ("carry", rcarry)):
        close_x3(part, f"{tag}:{nm}", o[nm], ref)


# ------------------------------------------------------------------ part P: the two-layer wavefront
@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 17, 33))
@pytest.mark.parametrize("H0,H1", [(24, 40), (40, 8), (264, 24)])
def test_lstm_pair_wavefront(NO, H0, H1, B):
    part = "P"
    for T in TS:
        tag = f"H{H0}-{H1}:B{B}:T{T}"
        r = Draw(27000 + 100 * H0 + 10 * H1 + 4 * B + T)
        v0 = _lstm_inputs(r, B, T, H0)
        v1 = _lstm_inputs(r, B, T, H1)
        W1, b1 = r.w(4 * H1, H0), r.n(4 * H1, dt=f32)
        g = Guard()

        def saves(H):
            return dict(out=g.new((B, T, H), bf), cs=g.new((T, B, H), f32), acts=g.new((T, B, 4 * H), f32),
                        tcs=g.new((T, B, H), f32), DG=g.new((B, T, 4 * H), bf), gc=g.new((B, H), f32))
        o0, o1 = saves(H0), saves(H1)
        c00, c01 = dev(v0["c0"]), dev(v1["c0"])
        NO.lstm2_seq_forward(dev(v0["x2"]), dev(v0["h0"]), c00, dev(v0["U"]), o0["out"], o0["cs"], o0["acts"],
                             o0["tcs"], None, dev(b1), dev(W1), dev(v1["h0"]), c01, dev(v1["U"]), o1["out"], o1["cs"],
                             o1["acts"], o1["tcs"], None)
        NO.lstm2_seq_backward(dev(v1["gy"]), dev(tr(v1["U"])), o1["acts"], o1["tcs"], o1["cs"], c01, o1["DG"],
                              o1["gc"], dev(tr(v0["U"])), dev(tr(W1)), o0["acts"], o0["tcs"], o0["cs"], c00, o0["DG"],
                              o0["gc"])
        g.check()
        # layer 1's input projection from layer 0's device output; layer 0's dh source from layer 1's device DG
        x21 = d(b1) + d(o0["out"]) @ d(W1).t()
        gy0 = d(o1["DG"]) @ d(W1)
        for L, v, o, x2, gy, H in ((0, v0, o0, d(v0["x2"]), gy0, H0), (1, v1, o1, x21, d(v1["gy"]), H1)):
            U = d(v["U"])
            out, cs, acts, tcs = lstm_fwd(x2, d(v["h0"]), d(v["c0"]), U, forced=d(o["out"]))
            rDG, rgc = lstm_bwd(gy, U, acts, tcs, cs, d(v["c0"]), forced=d(o["DG"]))
            for t in range(T):
                close_bf16(part, f"{tag}:out{L}[{t}]", o["out"][:, t], out[:, t])
                close_f32(part, f"{tag}:cs{L}[{t}]", o["cs"][t], cs[t])
                close_f32(part, f"{tag}:tcs{L}[{t}]", o["tcs"][t], tcs[t])
                for k, nm in enumerate("igfo"):
                    sl = slice(k * H, (k + 1) * H)
                    close_f32(part, f"{tag}:acts{L}_{nm}[{t}]", o["acts"][t][:, sl], acts[t][:, sl])
                    close_bf16(part, f"{tag}:DG{L}_{nm}[{t}]", o["DG"][:, t, sl], rDG[:, t, sl])
            close_f32(part, f"{tag}:gc{L}", o["gc"], rgc)
