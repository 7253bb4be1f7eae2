"""The MFMA GEMM (gemm.hip: k_gemm<64,64,64>, k_gemm<128,128,64>, the split-K slabs and their epilogue
kernel) in the forms the recurrent layer calls it and at its tile / k-tile / slice edges, against fp64.

Reference: fp64 ``act(alpha·A·Bᵀ + bias + D + beta·C)`` on the bf16-rounded operands (beta·C enters before
the activation, as gemm.hip documents); sigmoid / tanh are ``torch.sigmoid`` / ``torch.tanh`` in fp64.
Operands are drawn in fp32 on the host and rounded once; B is N(0, 1/K) so the product is O(1).

Bounds (none taken from the code under test):
  bf16 out   per element |got − ref| ≤ 2⁻⁸·|ref| + 2e-5·rms(ref)   (bf16 unit roundoff + the
             fp32-accumulation allowance of tests/test_bf16_kernel_variants.py)
  fp32 out   |got − ref| ≤ 2e-5·rms(ref)
Basis of the allowance: the same products in torch fp32 on the host against fp64, max error / rms(ref):
  (129, 16388, 72) 1.1e-6, (33, 264, 1056) 6.2e-7, split-K (3, 12, 2056) 1.6e-7, (3, 12, 8200) 3.6e-7.
For the split-K shapes (K ≥ 2048) the allowance is max(2e-5, 2 × that figure) = 2e-5 as well.

Every ``out`` is a 16-byte-aligned slice of a buffer pre-filled with the byte 0x7F whose bytes outside the
slice (for a strided ``out``: outside its columns too) must be untouched after the call, and every test
asserts that nothing fell back to torch.

Worst observed fraction of each bound per case group on an MI355X (profiles/rnn_oracle_errors.txt), bf16 /
fp32: activations 0.989 / 0.011, recurrent calls 0.976 / 0.040, k tails 0.992 / 0.015, 128-tile 0.994 / 0.016,
split-K 0.788 / 0.008.
"""
import pytest
import torch

bf = torch.bfloat16
f32 = torch.float32

U_BF16 = 2.0 ** -8
ABS = 2e-5
SENT, PAD = 0x7F, 256


@pytest.fixture
def NO():
    from bigdl import ops
    from bigdl.ops import native_ops
    st = ops.native_status()
    assert st["loaded"], st
    ops.reset_fallbacks()
    yield native_ops
    assert ops.fallback_counts() == {}, ops.fallback_counts()


class Guard:
    """[M][N] outputs (row stride ld ≥ N) inside sentinel-filled buffers; ``check`` proves that only the
    M × N elements were written."""

    def __init__(self):
        self.items = []

    def new(self, M, N, dtype, ld=None, col0=0, init=None):
        ld = ld or N
        es = torch.empty((), dtype=dtype).element_size()
        n = M * ld * es
        buf = torch.full((PAD + n + PAD,), SENT, dtype=torch.uint8, device="cuda")
        t = buf[PAD:PAD + n].view(dtype).view(M, ld)[:, col0:col0 + N]
        if init is not None:
            t.copy_(init)
        mask = torch.ones(M, ld * es, dtype=torch.bool, device="cuda")
        mask[:, col0 * es:(col0 + N) * es] = False
        self.items.append((buf, n, mask))
        return t

    def check(self):
        torch.cuda.synchronize()
        for k, (buf, n, mask) in enumerate(self.items):
            assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), f"guard band {k} written"
            assert bool((buf[PAD:PAD + n].view(mask.shape)[mask] == SENT).all()), f"columns outside out {k} written"


def _report(part, what, frac):
    print(f"[gemm-oracle] part={part} what={what} frac={frac:.3e}")
    assert frac <= 1.0, (part, what, frac)


def close(part, what, got, ref):
    rel = U_BF16 if got.dtype == bf else 0.0
    got = got.double().cpu()
    assert got.shape == ref.shape
    rms = float(ref.pow(2).mean().sqrt())
    _report(part, what, float(((got - ref).abs() / (rel * ref.abs() + ABS * rms)).max()))


ACTS = {0: lambda v: v, 1: torch.relu, 2: torch.sigmoid, 3: torch.tanh}


def reference(a, b, bias=None, act=0, d=None, alpha=1.0, beta=0.0, c=None):
    v = alpha * (a.double().cpu() @ b.double().cpu().t())
    if bias is not None:
        v = v + bias.double().cpu()
    if d is not None:
        v = v + d.double().cpu()
    if beta:
        v = v + beta * c.double().cpu()
    return ACTS[act](v)


class Draw:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def n(self, *shape, scale=1.0, dt=bf):
        return (torch.randn(*shape, generator=self.g) * scale).to(dt).cuda()


def _both_outputs(NO, part, tag, a, b, r, act=0):
    """bf16 out with bias + act, fp32 out with the d / alpha / beta epilogue (+ act), of one A·Bᵀ."""
    M, N = a.shape[0], b.shape[0]
    bias, dd, c0 = r.n(N, dt=f32), r.n(M, N), r.n(M, N, dt=f32)
    g = Guard()
    y = g.new(M, N, bf)
    c = g.new(M, N, f32, init=c0)
    assert NO.gemm(a, b, bias, act=act, out=y) is y
    assert NO.gemm(a, b, None, act=act, out=c, d=dd, alpha=0.5, beta=2.0) is c
    g.check()
    close(part, tag + ":bf16", y, reference(a, b, bias, act))
    close(part, tag + ":fp32", c, reference(a, b, None, act, dd, 0.5, 2.0, c0))


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activations(NO, act):
    M, N, K = 37, 100, 72
    r = Draw(100 + act)
    _both_outputs(NO, "act", f"act{act}", r.n(M, K), r.n(N, K, scale=K ** -0.5), r, act)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H", [(1, 3, 8), (17, 3, 24), (33, 1, 264)])
def test_recurrent_layer_calls(NO, B, T, H):
    """gh = DG[:, 0]·U (strided A, M = B) and dh0 = carry + da_rz_0·U_rz into an fp32 out, beta = 1."""
    r = Draw(200 + H)
    tag = f"B{B}:T{T}:H{H}"
    g = Guard()
    DG, Ut = r.n(B, T, 4 * H), r.n(H, 4 * H, scale=(4 * H) ** -0.5)
    a = DG[:, 0]
    assert a.stride(0) == T * 4 * H
    y = g.new(B, H, bf)
    assert NO.gemm(a, Ut, out=y) is y
    DG3, Urz_t, c0 = r.n(B, T, 3 * H), r.n(H, 2 * H, scale=(2 * H) ** -0.5), r.n(B, H, dt=f32)
    a3 = DG3[:, 0, :2 * H]
    assert a3.stride(0) == T * 3 * H
    carry = g.new(B, H, f32, init=c0)
    assert NO.gemm(a3, Urz_t, out=carry, beta=1.0) is carry
    g.check()
    close("rnn", tag + ":gh", y, reference(a, Ut))
    close("rnn", tag + ":dh0", carry, reference(a3, Urz_t, beta=1.0, c=c0))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 56, 64, 72, 128, 136, 192])
def test_k_tails(NO, K):
    """KT = 1, 2, 3 k-tiles, each with and without a partial last tile; both exits of the two-ahead pipeline."""
    M, N = 70, 96
    r = Draw(300 + K)
    _both_outputs(NO, "ktail", f"K{K}", r.n(M, K), r.n(N, K, scale=K ** -0.5), r)


BIG = (129, 16388, 72)


@pytest.fixture(scope="module")
def big():
    """Operands and the fp64 product of the 128 × 128-tile shape, computed once."""
    M, N, K = BIG
    assert ((M + 127) // 128) * ((N + 127) // 128) >= 256
    r = Draw(400)
    a, wide = r.n(M, K), r.n(N, 2 * K, scale=K ** -0.5)
    return dict(a=a, b=wide[:, :K].contiguous(), wide=wide, r=r, prod=a.double().cpu() @ wide[:, :K].double().cpu().t())


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["bias_relu", "fp32_d_beta", "strided_out_d", "strided_b"])
def test_tile_128(NO, big, variant):
    M, N, K = BIG
    a, b, r = big["a"], big["b"], big["r"]
    g = Guard()
    if variant == "bias_relu":
        bias = r.n(N, dt=f32)
        y = g.new(M, N, bf)
        NO.gemm(a, b, bias, act=1, out=y)
        ref = torch.relu(big["prod"] + bias.double().cpu())
    elif variant == "fp32_d_beta":
        dd, c0 = r.n(M, N), r.n(M, N, dt=f32)
        y = g.new(M, N, f32, init=c0)
        NO.gemm(a, b, None, out=y, d=dd, alpha=0.5, beta=2.0)
        ref = 0.5 * big["prod"] + dd.double().cpu() + 2.0 * c0.double().cpu()
    elif variant == "strided_out_d":
        dd = r.n(M, N + 24)[:, 8:8 + N]
        y = g.new(M, N, bf, ld=N + 12, col0=4)
        assert y.stride(0) > N and dd.stride(0) > N
        NO.gemm(a, b, None, out=y, d=dd)
        ref = big["prod"] + dd.double().cpu()
    else:
        bv = big["wide"][:, :K]
        assert bv.stride(0) == 2 * K
        y = g.new(M, N, bf)
        NO.gemm(a, bv, None, out=y)
        ref = big["prod"]
    g.check()
    close("tile128", variant, y, ref)


def _launcher_slices(K, S):
    """Slices the launcher really runs for ``S`` requested ones: whole 64-wide k-tiles per slice."""
    per = ((K + 63) // 64 + S - 1) // S
    return (K + per * 64 - 1) // (per * 64)


@pytest.mark.gpu
@pytest.mark.parametrize("K,asked,used", [(2056, 4, 4), (8200, 16, 15)])
def test_split_k(NO, K, asked, used):
    M, N = 3, 12
    assert NO._gemm_splits(M, N, K) == asked and _launcher_slices(K, asked) == used
    if K == 2056:  # the last slice holds 5 k-tiles + 8 columns
        per = ((K + 63) // 64 + asked - 1) // asked
        assert K - (used - 1) * per * 64 == 5 * 64 + 8
    r = Draw(500 + K)
    _both_outputs(NO, "splitk", f"K{K}", r.n(M, K), r.n(N, K, scale=K ** -0.5), r, act=1)
