"""The LARS kernels (``ops/csrc/lars.hip``) and the LarsPlan on the GPU.

* ``lars_sumsq`` + fold against fp64 sums on an awkward layer table, bitwise reproducible;
* ``lars_step`` against ``reference.lars_step`` from the same sums;
* a ``LocalOptimizer`` with the per-module LARS dict updates without one host synchronisation and
  lands on the weights of the per-method ``LarsSGD.optimize`` loop (a CPU twin);
* a world-1 ``DistriOptimizer`` runs the dict sharded and matches a ``LocalOptimizer``.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lars_sharded import awkward_case, step64, sums64  # noqa: E402
from test_distri_ptb import B, _mlp, _mlp_data, _weights  # noqa: E402


def _g(case, g_dtype):
    return case["g"].to(g_dtype).contiguous()


# The addition depth d of one layer sum is derived above k_lars_sumsq in csrc/lars.hip: d = 27 at the
# table's 8192-element chunks for a layer of up to 64 chunks (the longest layer here has 4).  Every
# term is non-negative, so the relative error is at most 27 · 2⁻²⁴ ≈ 1.6e-6; the bound below leaves
# about 6× headroom.
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_sumsq_fold_matches_fp64(g_dtype):
    from bigdl.ops import native_ops as NO
    from bigdl.utils import config
    c = awkward_case("cuda")
    w, g, t = c["w"], _g(c, g_dtype), c["table"]
    assert t.chunk == 8192 and t.n_chunks == 7 + 4  # seven one-chunk pieces and the four chunks of the long layer
    ref = sums64(c, w.cpu(), g.float().cpu()).reshape(-1)
    sums = NO.lars_sumsq(w, g, t)
    assert sums is not NotImplemented
    got = sums.double().cpu()
    for l in range(c["L"]):
        for k in (0, 1):
            r, v = float(ref[2 * l + k]), float(got[2 * l + k])
            rel = abs(v - r) / r if r > 0 else abs(v)
            print(f"layer {l} {'wg'[k]}: fp64 {r:.9e} kernel {v:.9e} rel {rel:.2e}")
            assert rel <= 1e-5, (l, k, r, v)
    o = c["outside"]
    assert float(got[2 * o]) == 0.0 and float(got[2 * o + 1]) == 0.0
    assert float(got[2 * c["zero_w"]]) == 0.0 and float(got[2 * c["zero_g"] + 1]) == 0.0
    # bitwise reproducible, with or without bigdl.deterministic
    again = NO.lars_sumsq(w, g, t, torch.empty_like(sums))
    assert torch.equal(again, sums)
    old = config.get_property("bigdl.deterministic")
    config.set_property("bigdl.deterministic", not old)
    try:
        assert torch.equal(NO.lars_sumsq(w, g, t), sums)
    finally:
        config.set_property("bigdl.deterministic", old)


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_shadow", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_lars_step_matches_reference(momentum, with_shadow, g_dtype):
    from bigdl.ops import native_ops as NO
    from bigdl.ops import reference as R
    c = awkward_case("cuda")
    t, g = c["table"], _g(c, g_dtype)
    hyper = c["hyper"].clone()
    hyper[:, 2] = momentum
    scale = 0.5
    sums = R.lars_sumsq(c["w"], g, t)  # both sides read the same sums
    w_ref, v_ref = c["w"].clone(), c["v"].clone()
    sh_ref = torch.full((c["n"],), 7.0, dtype=torch.bfloat16, device="cuda") if with_shadow else None
    R.lars_step(w_ref, g, v_ref, t, sums, hyper, scale, sh_ref)
    w, v = c["w"].clone(), c["v"].clone()
    sh = torch.full((c["n"],), 7.0, dtype=torch.bfloat16, device="cuda") if with_shadow else None
    assert NO.lars_step(w, g, v, t, sums, hyper, scale, sh) is not NotImplemented
    torch.testing.assert_close(w, w_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(v, v_ref, rtol=1e-5, atol=1e-6)
    own = torch.zeros(c["n"], dtype=torch.bool, device="cuda")
    for ss in c["spans"]:
        for a, b in ss:
            own[a:b] = True
    assert bool(own.any()) and bool((~own).any())
    # the update moved every owned element of a layer with a gradient, and nothing else
    assert torch.equal(w[~own], c["w"][~own]) and torch.equal(v[~own], c["v"][~own])
    if with_shadow:
        assert torch.equal(sh[own], w[own].to(torch.bfloat16))
        assert bool((sh[~own] == 7.0).all())
    # the two zero-norm layers take the ratio = 1 branch: the plain lr (column 3), no trust factor
    w64, v64, branch = step64(c, c["w"], g.float(), c["v"], sums, hyper, scale)
    for l in (c["zero_w"], c["zero_g"]):
        assert not branch[l]
        for a, b in c["spans"][l]:
            torch.testing.assert_close(w[a:b].double().cpu(), w64[a:b], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(v[a:b].double().cpu(), v64[a:b], rtol=1e-5, atol=1e-6)
    # a chunk sub-range (one owned range) updates exactly that range
    w2, v2 = c["w"].clone(), c["v"].clone()
    c0, c1 = t.chunk_range(*c["owned"][1])
    assert 0 < c0 < c1 == t.n_chunks
    assert NO.lars_step(w2, g, v2, t, sums, hyper, scale, None, c0, c1) is not NotImplemented
    lo = c["owned"][1][0]
    assert torch.equal(w2[:lo], c["w"][:lo]) and torch.equal(w2[lo:], w[lo:]) and torch.equal(v2[lo:], v[lo:])


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from bigdl.ops import native_ops as NO
    c = awkward_case("cuda")
    w, g, v, t = c["w"], c["g"], c["v"], c["table"]
    sums = torch.zeros(2 * c["L"], device="cuda")
    assert NO.lars_sumsq(w[1:], g[1:], t) is NotImplemented               # not the table's space
    assert NO.lars_sumsq(w, g.double(), t) is NotImplemented
    assert NO.lars_step(w, g, v, t, sums, c["hyper"][:, :3].contiguous(), 1.0) is NotImplemented
    assert NO.lars_step(w, g, v, t, sums, c["hyper"], 1.0, None, 0, t.n_chunks + 1) is NotImplemented
    assert NO.lars_step(w, g, v[:-1], t, sums, c["hyper"], 1.0) is NotImplemented
    assert torch.equal(w, awkward_case("cuda")["w"])


def _lars_dict(model):
    from bigdl.optim import LarsSGD
    return LarsSGD.createOptimForModule(model, learningRate=0.05, learningRateDecay=0.01, weightDecay=1e-3,
                                        momentum=0.9)


def _local(device):
    from bigdl.nn import ClassNLLCriterion
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    from bigdl.utils.engine import Engine
    Engine.init(device=device)
    model = _mlp()
    x, y = _mlp_data()
    x, y = x.to(device), y.to(device)
    opt = LocalOptimizer(model, [MiniBatch(x, y)], ClassNLLCriterion(), _lars_dict(model))
    opt.prepare()
    return opt, model, MiniBatch(x, y)


def test_local_optimizer_update_does_not_synchronise():
    from bigdl import ops
    from bigdl.optim.lars import _RING
    # more steps than staging rows, so the reuse of a row runs under the guard too
    steps = _RING + 2
    grads = [torch.randn(212, generator=torch.Generator().manual_seed(20 + i)) * 0.1 for i in range(steps)]
    # the oracle: the per-method LarsSGD.optimize loop on the CPU
    twin, twin_model, _ = _local("cpu")
    assert twin._lars_plan is None and twin.flat.grad.numel() == 212
    for g in grads:
        twin.flat.grad.copy_(g)
        twin._sync_and_update(torch.zeros(()), B)
    ref = _weights(twin_model)
    opt, model, _ = _local("cuda:0")
    assert opt._lars_plan is not None and opt._lars_plan.n_layers == 2
    w0 = _weights(model).cpu()
    dev_grads = [g.cuda() for g in grads]
    loss = torch.zeros((), device="cuda")
    ops.reset_fallbacks()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for g in dev_grads:
            opt.flat.grad.copy_(g)
            opt._sync_and_update(loss, B)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert not [k for k in ops.fallback_counts() if k[0].startswith("lars")]  # the HIP kernels ran
    got = _weights(model).cpu()
    assert not torch.equal(got, w0)
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-5)
    assert [m.state["evalCounter"] for m in opt.optim_methods.values()] == [steps, steps]


def test_world1_distri_optimizer_runs_lars_sharded():
    from bigdl.nn import ClassNLLCriterion
    from bigdl.dataset import MiniBatch
    from bigdl.parallel import DistriOptimizer
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    keys = ("bigdl.deterministic", "bigdl.comm.sharded", "bigdl.comm.bucketMB")
    old = {k: config.get_property(k) for k in keys}
    config.set_property("bigdl.deterministic", True)
    config.set_property("bigdl.comm.sharded", True)
    config.set_property("bigdl.comm.bucketMB", 0.0005)  # two buckets
    try:
        ref_opt, ref_model, batch = _local("cuda:0")
        for _ in range(3):
            ref_opt.train_step(batch)
        ref_opt._finish()
        ref = _weights(ref_model).cpu()
        Engine.init(device="cuda:0")
        model = _mlp()
        w0 = _weights(model)
        opt = DistriOptimizer(model, [batch], ClassNLLCriterion(), _lars_dict(model))
        opt.prepare()
        assert opt.sharded and opt._alias and len(opt.buckets) == 2
        assert opt._lars_plan is not None and opt._lars_plan.v.numel() == opt.shard_w.numel()
        for _ in range(3):
            opt.train_step(batch)
        opt._finish()
        torch.cuda.synchronize()
        got = _weights(model).cpu()
    finally:
        for k, v in old.items():
            config.set_property(k, v)
    assert not torch.equal(got, w0)
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-5)
