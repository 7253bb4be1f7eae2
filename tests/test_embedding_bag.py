"""The fused embedding-bag kernels (csrc/embedding_bag.hip) behind LookupTableSparse against ``bag``, a torch
form written from ``DL/nn/LookupTableSparse.scala:77-159``.  ``bag`` in fp64 on the table as stored (bf16 widened) is
the oracle, its autograd the gradWeight oracle (clip term included); ``bag`` in fp32 on the host gives the yardstick
E_fp32 per tensor, and the kernels must stay within 4·E_fp32 + 1e-6 (the bound of test_optim_fused.py).  Every case
prints its fraction of the bound (``pytest -m gpu -s``); profiles/embedding_bag_errors.txt keeps the worst per part.
"""
import functools

import pytest
import torch

from bigdl import ops
from bigdl.nn import LookupTableSparse
from bigdl.utils import config
from bigdl.utils.engine import Engine

pytestmark = pytest.mark.gpu
N_INDEX, N_BAGS, L = 50, 80, 70
DS = (1, 3, 8, 40, 200, 520)
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def bag(W, ids_per_bag, wts, combiner, max_norm):
    out = []
    for b, ids in enumerate(ids_per_bag):
        if not ids:
            out.append(W.new_zeros(W.shape[1]))
            continue
        E = W[torch.tensor(ids) - 1]
        w = W.new_ones(len(ids)) if wts is None else torch.tensor(wts[b], dtype=W.dtype)
        scale = w if combiner == "sum" else (w / w.sum() if combiner == "mean" else w / (w * w).sum().sqrt())
        if max_norm > 0:
            nrm = E.norm(dim=1)
            scale = scale * torch.where(nrm > max_norm, max_norm / nrm, torch.ones_like(nrm))
        out.append((scale.unsqueeze(1) * E).sum(0))
    return torch.stack(out)


@functools.lru_cache(None)
def layout():
    """80 bags over 50 ids: empty, one id, 70 ids, one id three times, id 7 in every non-empty bag (a run of >= 78:
    three 32-chunks of the sorted backward), ids 1 and 50; per-id weights, and a copy with one zero weight."""
    g = torch.Generator().manual_seed(7)
    bags = [[], [7], [7, 50, 1] + torch.randint(1, N_INDEX + 1, (67,), generator=g).tolist(), [7, 3, 3, 3]]
    while len(bags) < N_BAGS:
        bags.append([7] + torch.randint(1, N_INDEX + 1, (int(torch.randint(1, 6, (1,), generator=g)),),
                                        generator=g).tolist())
    wts = [(torch.rand(len(b), generator=g) + 0.5).tolist() for b in bags]
    wz = [list(w) for w in wts]
    wz[3][1] = 0.0
    return bags, {"none": None, "given": wts, "zero": wz}


@functools.lru_cache(None)
def table(D, dt):
    W = torch.randn(N_INDEX, D, generator=torch.Generator().manual_seed(1234 + D)).to(DT[dt])
    nrm = W.double().norm(dim=1).sort().values
    mid = nrm[15:35]
    k = int((mid[1:] - mid[:-1]).argmax())
    m = float((mid[k] + mid[k + 1]) / 2)
    assert float(((nrm / m) - 1).abs().min()) > 1e-3  # guard band: no row norm near the threshold
    return W, m


@functools.lru_cache(None)
def reference(D, dt, gdt, comb, wmode, clip):
    """(gy, gw0, oracle out, oracle gw, bound out, bound gw) for scale 0.5 into a non-zero gradWeight."""
    W, m = table(D, dt)
    bags, wts = layout()
    g = torch.Generator().manual_seed(99 + D)
    gy = torch.randn(N_BAGS, D, generator=g).to(DT[gdt])
    gw0 = torch.randn(N_INDEX, D, generator=g)
    res = []
    for prec in (torch.float64, torch.float32):
        Wp = W.to(prec).clone().requires_grad_()
        out = bag(Wp, bags, wts[wmode], comb, m if clip else -1.0)
        out.backward(gy.to(prec))
        res += [out.detach(), gw0.to(prec) + 0.5 * Wp.grad]
    bo = 4 * float((res[2].double() - res[0]).abs().max()) + 1e-6
    bg = 4 * float((res[3].double() - res[1]).abs().max()) + 1e-6
    return gy, gw0, res[0], res[1], bo, bg


def inputs(wmode, form):
    bags, wts = layout()
    w = wts[wmode]
    if form == "dense":
        ids = torch.tensor([b + [0] * (L - len(b)) for b in bags], dtype=torch.float32).cuda()
        wt = None if w is None else torch.tensor([x + [0.0] * (L - len(x)) for x in w]).cuda()
        return ids, None, L, wt
    rows = torch.tensor([b for b, x in enumerate(bags) for _ in x]).cuda()
    ids = torch.tensor([i for x in bags for i in x]).cuda()
    return ids, rows, N_BAGS, (None if w is None else torch.tensor([v for x in w for v in x]).cuda())


def check(name, got, want, bound):
    err = float((got.double().cpu() - want).abs().max())
    print(f"EB {name} err={err:.3e} bound={bound:.3e} frac={err / bound:.3f}")
    assert err <= bound, (name, err, bound)


def run_case(D, dt, gdt, comb, wmode, clip):
    W, m = table(D, dt)
    gy, gw0, o_out, o_gw, bo, bg = reference(D, dt, gdt, comb, wmode, clip)
    Wd, gyd, res = W.cuda(), gy.cuda(), {}
    for form in ("coo", "dense"):
        for rep in range(2):
            out, st = ops.embedding_bag_forward(Wd, *inputs(wmode, form), comb, m if clip else -1.0)
            gw = gw0.cuda()
            ops.embedding_bag_backward(gw, st, gyd, Wd, 0.5)
            res[form, rep] = (out, gw)
    ops.embedding_check(sync=True)
    tag = f"D{D}:{dt}:gy{gdt}:{comb}:{wmode}:{'clip' if clip else 'noclip'}"
    check(f"part=fwd {tag}", res["coo", 0][0], o_out, bo)
    check(f"part=bwd {tag}", res["coo", 0][1], o_gw, bg)
    for k in (("coo", 1), ("dense", 0), ("dense", 1)):  # same bits: both input forms, every launch
        assert torch.equal(res[k][0], res["coo", 0][0]) and torch.equal(res[k][1], res["coo", 0][1]), k


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("wmode", ["none", "given", "zero"])
@pytest.mark.parametrize("comb", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("D", DS)
def test_kernels(D, dt, comb, wmode, clip):
    run_case(D, dt, "fp32", comb, wmode, clip)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [8, 200])
def test_kernels_bf16_gy(D, dt):
    run_case(D, dt, "bf16", "mean", "given", True)


def layer_run(dt, form, wmode, clip, native, D=40):
    """forward / backward of a LookupTableSparse on the device; (out, gradWeight as scale 0.5 into gw0)."""
    from bigdl.utils.table import Table
    W, m = table(D, dt)
    gy, gw0 = reference(D, dt, "fp32", "mean", wmode, clip)[:2]
    config.set_property("bigdl.compute.dtype", dt)
    config.set_property("bigdl.embedding.nativeBag", native)
    try:
        Engine.init(device="cuda:0")
        mod = LookupTableSparse(N_INDEX, D, "mean", m if clip else -1.0)
        mod.weight.copy_(W.float())
        mod = mod.cuda()
        mod.gradWeight.copy_(gw0.cuda())
        mod.setScaleW(0.5)
        ids, rows, n, wt = inputs(wmode, form)
        if rows is not None:
            cols = torch.cat([torch.arange(len(b)) for b in layout()[0]]).cuda()
            idx = torch.stack([rows, cols])
            ids = torch.sparse_coo_tensor(idx, ids.float(), (N_BAGS, L))
            wt = None if wt is None else torch.sparse_coo_tensor(idx, wt, (N_BAGS, L))
        x = ids if wt is None else Table(ids, wt)
        out = mod.forward(x)
        mod.backward(x, gy.cuda())
        return out, mod.gradWeight.clone()
    finally:
        config.clear_property("bigdl.compute.dtype")
        config.clear_property("bigdl.embedding.nativeBag")


@pytest.mark.parametrize("dt,form,wmode", [("fp32", "coo", "given"), ("bf16", "dense", "none")])
def test_layer(dt, form, wmode):
    for clip in (True, False):
        _, _, o_out, o_gw, bo, bg = reference(40, dt, "fp32", "mean", wmode, clip)
        out, gw = layer_run(dt, form, wmode, clip, True)
        assert out.dtype == torch.float32
        check(f"part=layer-fwd {dt}:{form}:clip{int(clip)}", out, o_out, bo)
        check(f"part=layer-bwd {dt}:{form}:clip{int(clip)}", gw, o_gw, bg)
    # the torch form of the same module (it reads the fp32 master: compare on a table bf16 holds exactly)
    t_out, t_gw = layer_run(dt, form, wmode, False, False)
    check(f"part=layer-vs-torch-fwd {dt}:{form}", out, t_out.double().cpu(), bo)
    check(f"part=layer-vs-torch-bwd {dt}:{form}", gw, t_gw.double().cpu(), bg)


def test_bad_id_raises_and_process_goes_on():
    W = table(8, "fp32")[0].cuda()
    ids = torch.tensor([[3.0, N_INDEX + 1.0, 0.0]]).cuda()
    out, _ = ops.embedding_bag_forward(W, ids, None, 3, None, "sum", -1.0)
    with pytest.raises(IndexError):
        ops.embedding_check(sync=True)
    assert torch.equal(out[0], W[2] + W[N_INDEX - 1])  # the id was clamped: nothing faulted
    ops.embedding_check(sync=True)
