"""Sharded, sync-free LARS (``optim/lars.py``, ``ops.lars_sumsq`` / ``ops.lars_step``) on the CPU.

* the per-module constructors of ``LarsSGD`` (``LarsSGD.scala:163-282``);
* the torch reference ops against an explicit per-layer fp64 loop on an awkward layer table;
* a ``DistriOptimizer`` at gloo world 2 with the per-module LARS dict runs SHARDED and matches a
  serial ``LocalOptimizer`` on the whole batch (whose ``LarsSGD.optimize`` loop is the oracle);
* the plan's momentum buffer survives ``export_state`` / ``import_state`` bit for bit.
"""
import copy
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from test_distri_cpu import _free_port
from test_distri_ptb import B, _mlp, _mlp_data, _weights


# ------------------------------------------------------------------------------------------ API
def test_create_optim_for_module_api():
    from bigdl.nn import Sequential, Linear, Tanh, LogSoftMax, ClassNLLCriterion
    from bigdl.optim import LarsSGD, SGD, Adam, Step
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    from bigdl.utils.engine import Engine
    Engine.init(device="cpu")
    l1, l2, l3 = Linear(8, 16), Linear(16, 6), Linear(6, 4)
    inner = Sequential().add(Tanh()).add(l2).add(Tanh())
    model = Sequential().add(l1).add(inner).add(l3).add(LogSoftMax())
    sched = Step(10, 0.5)
    d = LarsSGD.createOptimForModule(model, trust=0.9, learningRate=0.1, learningRateDecay=0.0, weightDecay=1e-3,
                                     momentum=0.9, learningRateSchedule=sched)
    assert list(d) == [l1.get_name(), l2.get_name(), l3.get_name()]
    assert all(type(m) is LarsSGD for m in d.values())
    assert all(m.learningRateSchedule is sched for m in d.values())
    assert all((m.trust, m.learningRate, m.weightDecay, m.momentum) == (0.9, 0.1, 1e-3, 0.9) for m in d.values())
    hyper = [m.getHyperParameter() for m in d.values()]
    assert hyper[0] != "" and hyper[1:] == ["", ""]
    # defaults: one shared Default schedule
    d0 = LarsSGD.createOptimForModule(model)
    assert len({id(m.learningRateSchedule) for m in d0.values()}) == 1
    assert sum(1 for m in d0.values() if m.getHyperParameter()) == 1
    # a generator decides schedule and ownership per module
    seen = []

    def gen(mod):
        seen.append(mod.get_name())
        return Step(5, 0.1), mod is l3
    d2 = LarsSGD.createOptimLRSchedulerForModule(model, gen, weightDecay=0.25)
    assert seen == list(d) and list(d2) == list(d)
    assert len({id(m.learningRateSchedule) for m in d2.values()}) == 3
    assert [bool(m.getHyperParameter()) for m in d2.values()] == [False, False, True]
    assert LarsSGD.containsLarsSGD(d2) == 0.25
    assert LarsSGD.containsLarsSGD({"a": SGD(), "b": LarsSGD(weightdecay=0.125), "c": LarsSGD(weightdecay=0.5)}) == 0.125
    assert LarsSGD.containsLarsSGD({"a": SGD(), "b": Adam()}) is None
    # the flags the drivers consult
    assert LarsSGD.supports_layer_shards and not LarsSGD.supports_slices
    assert LarsSGD().prepare_graph() is False
    # the dict covers every parameter: a LocalOptimizer takes it
    x, y = torch.randn(B, 8), (torch.randint(0, 4, (B,)) + 1).float()
    w0 = _weights(model)
    opt = LocalOptimizer(model, [MiniBatch(x, y)], ClassNLLCriterion(), d)
    opt.prepare()
    opt.train_step(MiniBatch(x, y))
    assert not torch.equal(_weights(model), w0)
    assert all(m.state["evalCounter"] == 1 for m in d.values())  # each method's own counter advanced
    assert opt._hyper_str().count("Current learning rate") == 1


# ------------------------------------------------------------------------------------------ awkward table
def awkward_case(device="cpu", chunk=None, seed=0):
    """Layers of awkward lengths laid back to back, an owned range that starts inside a layer at an
    offset ≡ 1 (mod 4) and ends inside another, a layer wholly outside, a layer with w = 0 and one
    with g = 0.  Returns a dict with the table, the tensors and the per-layer owned spans."""
    from bigdl.ops.lars_table import LarsTable
    chunk = chunk or LarsTable.CHUNK
    lens = [3, 255, 1, 5, 257, 4095, 256, 3 * chunk + 7, 4097]
    offs = [sum(lens[:i]) for i in range(len(lens))]
    n = sum(lens)
    assert n < 70000 and {1, 2, 3} <= {o % 4 for o in offs}
    own_lo2 = offs[3] + 2                      # inside the layer of 5
    own_hi2 = offs[8] + 2001                   # inside the last layer
    assert own_lo2 % 4 == 1
    owned = [(0, offs[2]), (own_lo2, own_hi2)]  # layer 2 (one element) lies wholly outside
    spans = [[(max(o, lo), min(o + m, hi)) for lo, hi in owned if max(o, lo) < min(o + m, hi)]
             for o, m in zip(offs, lens)]
    assert spans[2] == [] and all(spans[i] for i in range(len(lens)) if i != 2)
    pieces = [(a, b - a, l) for l, ss in enumerate(spans) for a, b in ss]
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.1
    w[offs[6]:offs[6] + lens[6]] = 0          # zero weight norm
    gr[offs[4]:offs[4] + lens[4]] = 0         # zero gradient norm
    v = torch.randn(n, generator=g) * 0.01
    L = len(lens)
    hyper = torch.tensor([[0.05 * (0.5 + 0.1 * l), 1e-3 * (l % 3), 0.9, 0.1] for l in range(L)])
    return {"table": LarsTable(pieces, L, n, device, chunk), "w": w.to(device), "g": gr.to(device),
            "v": v.to(device), "hyper": hyper.to(device), "spans": spans, "n": n, "L": L, "owned": owned,
            "zero_w": 6, "zero_g": 4, "outside": 2}


def sums64(case, w, g):
    """fp64 (Σw², Σg²) of every layer's owned part: [L, 2]."""
    out = torch.zeros(case["L"], 2, dtype=torch.float64)
    for l, ss in enumerate(case["spans"]):
        for a, b in ss:
            out[l, 0] += w[a:b].double().square().sum().cpu()
            out[l, 1] += g[a:b].double().square().sum().cpu()
    return out


def step64(case, w, g, v, sums, hyper, grad_scale):
    """The update of ``LarsSGD.optimize`` layer by layer in fp64, from the given sums; returns
    (w, v) as fp64 tensors (elements outside the owned spans unchanged)."""
    w, g, v = w.double().cpu().clone(), g.double().cpu(), v.double().cpu().clone()
    s, h = sums.double().cpu().reshape(-1, 2), hyper.double().cpu()
    branch = []
    for l, ss in enumerate(case["spans"]):
        wn, gn = float(s[l, 0].sqrt()), grad_scale * float(s[l, 1].sqrt())
        lrt, wd, mom, lr = (float(t) for t in h[l])
        lars = wn > 0 and gn > 0
        branch.append(lars)
        rate = lrt * wn / (gn + wd * wn + 1e-12) if lars else lr
        for a, b in ss:
            v[a:b] = mom * v[a:b] + rate * (g[a:b] * grad_scale + wd * w[a:b])
            w[a:b] -= v[a:b]
    return w, v, branch


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_reference_ops_match_fp64_loop(g_dtype):
    from bigdl.ops import reference as R
    c = awkward_case(chunk=1000)
    w, v, hyper, t = c["w"], c["v"], c["hyper"], c["table"]
    g = c["g"].to(g_dtype)
    assert t.n_chunks > len(c["spans"]) and max(t.lens) <= 1000
    ref = sums64(c, w, g.float())
    sums = R.lars_sumsq(w, g, t)
    assert sums.dtype == torch.float32 and sums.shape == (2 * c["L"],)
    # accumulated in fp64 and rounded once: half an ulp of fp32
    torch.testing.assert_close(sums.double().reshape(-1, 2), ref, rtol=2.0 ** -23, atol=0)
    assert sums[2 * c["outside"]] == 0 and sums[2 * c["outside"] + 1] == 0
    w0, v0 = w.clone(), v.clone()
    w64, v64, branch = step64(c, w, g.float(), v, sums, hyper, 0.5)
    assert not branch[c["zero_w"]] and not branch[c["zero_g"]] and sum(branch) == c["L"] - 3
    shadow = torch.zeros(c["n"], dtype=torch.bfloat16)
    R.lars_step(w, g, v, t, sums, hyper, 0.5, shadow)
    torch.testing.assert_close(w.double(), w64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(v.double(), v64, rtol=1e-5, atol=1e-6)
    own = torch.zeros(c["n"], dtype=torch.bool)
    for ss in c["spans"]:
        for a, b in ss:
            own[a:b] = True
    assert torch.equal(w[~own], w0[~own]) and torch.equal(v[~own], v0[~own]) and not shadow[~own].any()
    assert torch.equal(shadow[own], w[own].to(torch.bfloat16))
    # a chunk sub-range updates exactly its chunks
    w2, v2 = w0.clone(), v0.clone()
    c0, c1 = t.chunk_range(*c["owned"][1])
    assert (c0, c1) == (t.chunk_range(0, c["owned"][0][1])[1], t.n_chunks)
    R.lars_step(w2, g, v2, t, sums, hyper, 0.5, None, c0, c1)
    lo = c["owned"][1][0]
    assert torch.equal(w2[:lo], w0[:lo]) and torch.equal(w2[lo:], w[lo:])


def test_table_rejects_bad_pieces():
    from bigdl.ops.lars_table import LarsTable
    with pytest.raises(ValueError):
        LarsTable([(0, 10, 0), (8, 4, 1)], 2, 100, "cpu")   # overlap
    with pytest.raises(ValueError):
        LarsTable([(95, 10, 0)], 1, 100, "cpu")             # leaves the space
    with pytest.raises(ValueError):
        LarsTable([(0, 10, 3)], 2, 100, "cpu")              # unknown layer


# ------------------------------------------------------------------------------------------ sharded == serial
def _convnet(world=1):
    """conv → BN → ReLU → Linear, 2796 parameters, sized so that at ``bucketMB = 0.002`` and world 2
    the first bucket closes after BN's γ: γ lands in rank 1's half of bucket 0 and β in rank 0's half
    of bucket 1 — the BN layer (2·C = 28 elements) is cut by a shard boundary."""
    from bigdl.nn import (Sequential, SpatialConvolution, SpatialBatchNormalization, ReLU, Reshape, Linear,
                          LogSoftMax)
    from bigdl.utils.random import RNG
    RNG.setSeed(9)
    torch.manual_seed(9)
    bn = SpatialBatchNormalization(14)
    bn.setParallism(world)  # SyncBN: the two half batches are the serial run's mathematics
    return (Sequential().add(SpatialConvolution(4, 14, 3, 3)).add(bn).add(ReLU())
            .add(Reshape([14 * 4 * 4])).add(Linear(14 * 4 * 4, 10)).add(LogSoftMax()))


def _conv_data():
    g = torch.Generator().manual_seed(4)
    return torch.randn(B, 4, 6, 6, generator=g), (torch.randint(0, 10, (B,), generator=g) + 1).float()


def _setup(kind, world=1):
    from bigdl.nn import ClassNLLCriterion
    if kind == "conv":
        return _convnet(world), _conv_data(), ClassNLLCriterion()
    return _mlp(), _mlp_data(), ClassNLLCriterion()


def _methods(model, which):
    from bigdl.optim import LarsSGD, SGD
    d = LarsSGD.createOptimForModule(model, learningRate=0.05, learningRateDecay=0.01, weightDecay=1e-3,
                                     momentum=0.9)
    if which == "mixed":  # plain SGD on the first layer, LARS on the rest
        first = next(iter(d))
        d[first] = SGD(learningrate=0.05, learningrate_decay=0.01, weightdecay=1e-3, momentum=0.9, dampening=0.0)
    return d


def _worker(rank, world, port, kind, which, comm_dtype, steps, out_q):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bigdl-1_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="2")
    torch.set_num_threads(2)
    from bigdl.utils import config
    config.set_property("bigdl.comm.sharded", True)
    config.set_property("bigdl.comm.dtype", comm_dtype)
    config.set_property("bigdl.comm.bucketMB", 0.002)  # several buckets: shard boundaries split layers
    from bigdl.utils.engine import Engine
    Engine.init(device="cpu", dist=True, backend="gloo")
    from bigdl.parallel import DistriOptimizer
    from bigdl.dataset import MiniBatch
    from bigdl.optim import LarsSGD
    model, (x, y), crit = _setup(kind, world)
    per = x.shape[0] // world
    xs, ys = x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]
    methods = _methods(model, which)
    opt = DistriOptimizer(model, [MiniBatch(xs, ys)], crit, methods)
    opt.prepare()
    for _ in range(steps):
        opt.train_step(MiniBatch(xs, ys))
    opt._finish()
    if rank == 0:
        # elements of each method's parameters that THIS rank updates, and each method's size
        owned = {k: sum(hi - lo for (_b, lo, hi) in opt._method_shard_ranges[k]) for k in methods}
        sizes = {k: opt._method_slices[k][1] for k in methods}
        plan = opt._lars_plan
        out_q.put((bool(opt.sharded), _weights(model).numpy(), list(methods), owned, sizes,
                   plan is not None and plan.v.numel() == opt.shard_w.numel(),
                   [type(m).__name__ for m in methods.values() if plan.covers(m)],
                   [m.state.get("evalCounter") for m in methods.values()],
                   any(isinstance(m, LarsSGD) and isinstance(m.state.get("dfdx"), torch.Tensor)
                       for m in methods.values())))
    Engine.shutdown()


def _serial(kind, which, steps):
    from bigdl.optim.optimizer import LocalOptimizer
    from bigdl.dataset import MiniBatch
    from bigdl.utils.engine import Engine
    Engine.init(device="cpu")
    model, (x, y), crit = _setup(kind, 1)
    w0 = _weights(model)
    opt = LocalOptimizer(model, [MiniBatch(x, y)], crit, _methods(model, which))
    opt.prepare()
    assert opt._lars_plan is None  # CPU: the per-method LarsSGD.optimize loop, the oracle
    for _ in range(steps):
        opt.train_step(MiniBatch(x, y))
    return w0, _weights(model)


def _run(kind, which, comm_dtype, steps=3):
    w0, ref = _serial(kind, which, steps)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, kind, which, comm_dtype, steps, q)) for r in range(2)]
    for p in procs:
        p.start()
    sharded, got, names, owned, sizes, one_buffer, covered, counters, per_method_buf = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sharded, "the DistriOptimizer fell back to replicated mode"
    assert one_buffer and not per_method_buf  # ONE momentum buffer over the shard, none per LarsSGD
    assert covered == ["LarsSGD"] * (len(names) - (which == "mixed"))
    assert counters == [steps] * len(names)  # every method's evalCounter advanced once per step
    assert not torch.equal(ref, w0)  # the steps moved the weights
    return torch.from_numpy(got), ref, w0, names, owned, sizes


@pytest.mark.parametrize("kind", ["mlp", "conv"])
@pytest.mark.parametrize("comm_dtype", ["fp32", "bf16"])
def test_lars_sharded_matches_serial(kind, comm_dtype):
    got, ref, w0, names, owned, sizes = _run(kind, "lars", comm_dtype)
    # shard boundaries cut layers: some method is updated partly here, partly on the other rank
    assert any(0 < owned[k] < sizes[k] for k in names), (owned, sizes)
    if kind == "conv":
        bn = names[1]
        assert sizes[bn] > 28 and owned[bn] == 14, (owned, sizes)  # γ on rank 1, β on rank 0, padding between
    if comm_dtype == "fp32":
        torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-5)
    else:  # bf16 gradient wire: the update direction agrees, magnitudes within the wire's rounding
        cos = float(torch.nn.functional.cosine_similarity(got - w0, ref - w0, dim=0))
        assert cos > 0.99, cos


def test_mixed_sgd_and_lars_sharded_matches_serial():
    got, ref, _w0, _names, _owned, _sizes = _run("mlp", "mixed", "fp32")
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------ state round trip
def _plan_fixture():
    """Three LarsSGD 'modules' over a 600-element arena of which this 'rank' owns two groups
    (like two buckets' shards), mapped into a 300-element shard space; layer 1 is cut by both."""
    from bigdl.optim import LarsSGD
    slices = {"a": (0, 130), "b": (130, 333), "c": (463, 137)}
    owned = [(100, 250, 0, 0), (400, 550, 150, 1)]  # arena [lo, hi) → space offset, group

    def to_space(lo, hi):
        out = []
        for alo, ahi, soff, grp in owned:
            a, z = max(lo, alo), min(hi, ahi)
            if a < z:
                out.append((soff + a - alo, soff + z - alo, grp))
        return out
    methods = {k: LarsSGD(learningrate=0.05, learningrate_decay=0.01, weightdecay=1e-3, momentum=0.9)
               for k in slices}
    return methods, slices, to_space, 300


def _plan_steps(plan, w, steps, start=0):
    for i in range(start, start + steps):
        g = torch.randn(w.numel(), generator=torch.Generator().manual_seed(100 + i))
        plan.begin(w, g)
        for grp in (1, 0):
            plan.update(w, g, None, 0.5, group=grp)


def test_plan_state_round_trip():
    from bigdl.optim.lars import LarsPlan
    w_init = torch.randn(300, generator=torch.Generator().manual_seed(1))
    # three uninterrupted steps
    ma, slices, to_space, n = _plan_fixture()
    pa = LarsPlan(ma, slices, to_space, n, "cpu", chunk=64)
    wa = w_init.clone()
    _plan_steps(pa, wa, 3)
    # two steps, export, a fresh plan over the same layout from the (copied) methods, one more step
    mb, *_ = _plan_fixture()
    pb = LarsPlan(mb, slices, to_space, n, "cpu", chunk=64)
    wb = w_init.clone()
    _plan_steps(pb, wb, 2)
    assert pb.v.abs().sum() > 0
    pb.export_state()
    assert [m.state["dfdx"].numel() for m in mb.values()] == [30, 120 + 63, 87]
    mc = copy.deepcopy(mb)  # what a checkpoint restores: the methods with their state
    pc = LarsPlan(mc, slices, to_space, n, "cpu", chunk=64)
    assert torch.equal(pc.v, pb.v)
    assert all("dfdx" not in m.state for m in mc.values())  # consumed by the import
    pb.release_state()
    assert all("dfdx" not in m.state for m in mb.values())
    _plan_steps(pc, wb, 1, start=2)
    assert torch.equal(wb, wa) and torch.equal(pc.v, pa.v)
    assert [m.state["evalCounter"] for m in mc.values()] == [3, 3, 3]
    # a dfdx of another length is ignored
    md, *_ = _plan_fixture()
    md["a"].state["dfdx"] = torch.ones(31)
    assert not LarsPlan(md, slices, to_space, n, "cpu", chunk=64).v.any()


# ------------------------------------------------------------------------------------------ coverage on a padded arena
def test_method_coverage_on_a_bucketed_arena():
    """A bucketed arena holds padding that belongs to no parameter: a per-module dict that covers
    every parameter is accepted there, a dict with a gap or with overlapping methods is refused."""
    from bigdl.nn import ClassNLLCriterion
    from bigdl.dataset import MiniBatch
    from bigdl.optim import LarsSGD, SGD
    from bigdl.parallel import DistriOptimizer
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cpu")
    old = config.get_property("bigdl.comm.bucketMB")
    config.set_property("bigdl.comm.bucketMB", 0.0005)  # two buckets of the MLP, each padded
    try:
        x, y = _mlp_data()

        def prepared(methods_of):
            model = _mlp()
            opt = DistriOptimizer(model, [MiniBatch(x, y)], ClassNLLCriterion(), methods_of(model))
            opt.prepare()
            return opt, model
        opt, model = prepared(lambda m: LarsSGD.createOptimForModule(m))
        assert opt.flat.numel > sum(s[4] for s in opt.flat.slices) == 212  # there is padding
        assert sum(n for _o, n in opt._method_slices.values()) == 212

        def gap(m):
            d = LarsSGD.createOptimForModule(m)
            d.pop(next(iter(d)))
            return d

        def overlap(m):
            d = LarsSGD.createOptimForModule(m)
            d[m.get_name()] = SGD()  # the root covers everything, the layers again
            return d
        for bad in (gap, overlap):
            with pytest.raises(ValueError, match="exactly once"):
                prepared(bad)
    finally:
        config.set_property("bigdl.comm.bucketMB", old)
