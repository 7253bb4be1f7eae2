"""A/B of the LARS update phase on ResNet-50 (one GPU, no training data).

Three arms over the same parameter arena and the same seeded random gradient, alternating in one
process, ``--rounds`` rounds of ``--iters`` updates each after warm-up:

  (a) serial   the per-method ``LarsSGD.optimize`` loop (``bigdl.lars.fused=false``): two host
               reads of the layer norms per layer
  (b) plan     the LarsPlan: norm kernels + fold + one fused update, no host synchronisation
  (c) sgd      one ``ops.sgd_step`` with momentum over the whole arena (the bandwidth yardstick:
               20 B per element against the plan's 28 B, so (b)/(c) ≈ 1.4 from bytes alone)

Times are host wall-clock per update around a device synchronise (arm (a) is bound by its host
reads, so device events alone would miss what it costs).  Gate: (b) < (a) in every round.

    python tools/bench_lars.py [--out profiles/lars_update_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "bigdl-1_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "lars_update_ab.txt"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("bench_lars needs a GPU", file=sys.stderr)
        return 2
    from bigdl import ops
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.models.resnet import ResNet, DatasetType, model_init
    from bigdl.nn import CrossEntropyCriterion
    from bigdl.optim import LarsSGD
    from bigdl.optim.optimizer import LocalOptimizer
    Engine.init(device="cuda:0")

    def make(fused: bool):
        config.set_property("bigdl.lars.fused", fused)
        model = model_init(ResNet(1000, depth=a.depth, dataset=DatasetType.ImageNet))
        methods = LarsSGD.createOptimForModule(model, learningRate=0.1, learningRateDecay=0.0001, weightDecay=1e-4,
                                               momentum=0.9)
        opt = LocalOptimizer(model, None, CrossEntropyCriterion(), methods)
        opt.prepare()
        assert (opt._lars_plan is not None) == fused
        return opt, len(methods)

    opt_a, n_methods = make(False)
    opt_b, _ = make(True)
    n = opt_b.flat.numel
    grad = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1e-3
    for o in (opt_a, opt_b):
        o.flat.grad.copy_(grad)
    loss = torch.zeros((), device="cuda")
    # arm (c): plain momentum SGD over an arena of its own
    w_c = opt_b.flat.weight.clone()
    buf_c = torch.zeros_like(w_c)
    sh_c = torch.empty(n, dtype=torch.bfloat16, device="cuda") if opt_b.flat.shadow is not None else None

    def arm_a():
        opt_a._sync_and_update(loss, 1)

    def arm_b():
        opt_b._sync_and_update(loss, 1)

    def arm_c():
        ops.sgd_step(w_c, grad, buf_c, 0.1, 0.9, 0.0, 1e-4, False, False, 1.0, sh_c)

    arms = (("serial", arm_a), ("plan", arm_b), ("sgd", arm_c))
    for _ in range(a.warmup):
        for _name, f in arms:
            f()
    torch.cuda.synchronize()
    rows = []
    for r in range(a.rounds):
        row = {}
        for name, f in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            row[name] = (time.perf_counter() - t0) / a.iters * 1e3
        rows.append(row)
    fallbacks = [k for k in ops.fallback_counts() if k[0].startswith("lars")]
    lines = [f"LARS update phase, ResNet-{a.depth}: {n} arena elements, {n_methods} LarsSGD methods "
             f"({opt_b._lars_plan.table.n_chunks} chunks of <= {opt_b._lars_plan.table.chunk}), "
             f"shadow={'bf16' if sh_c is not None else 'none'}, {a.iters} updates per round after {a.warmup} warm-up",
             "ms per update (host wall-clock around a device synchronise), arms alternated in one process",
             f"{'round':>5} {'(a) serial':>11} {'(b) plan':>9} {'(c) sgd':>8} {'a/b':>7} {'b/c':>6}"]
    for i, row in enumerate(rows):
        lines.append(f"{i:>5} {row['serial']:>11.3f} {row['plan']:>9.3f} {row['sgd']:>8.3f} "
                     f"{row['serial'] / row['plan']:>7.2f} {row['plan'] / row['sgd']:>6.2f}")
    gate = all(row["plan"] < row["serial"] for row in rows)
    lines.append(f"gate (b) < (a) in every round: {'PASS' if gate else 'FAIL'}")
    lines.append(f"lars ops that fell back to torch: {fallbacks or 'none'}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if gate and not fallbacks else 1


if __name__ == "__main__":
    sys.exit(main())
