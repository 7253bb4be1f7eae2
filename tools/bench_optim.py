"""A/B of the update phase of the elementwise methods (one GPU, no model, no data).

A flat fp32 arena of ResNet-50's parameter count with a bf16 shadow and one seeded gradient.  For
each method two arms over arenas of their own, alternating in one process, ``--rounds`` rounds of
``--iters`` updates each after warm-up:

  (a) torch    the method's torch elementwise form (``bigdl.optim.fused=false``): a chain of
               launches with full-size temporaries plus the shadow cast
  (b) fused    the one-pass rule kernel (csrc/optim_rules.hip)

and, as the bandwidth yardstick, one momentum ``ops.sgd_step`` over the same arena: 20 B per
element (read w, g, v; write w, v) against 20 B for RMSprop and 28 B for the two-state methods, so
(b)/sgd should sit near 1.0 and 1.4 from bytes alone (the 2 B shadow write is in every arm).

Adagrad (20 B) and Adam (28 B) always take the kernel on the GPU (``bigdl.optim.fused`` does not
gate them), so their rows have arm (b) and the yardstick only.

Times are host wall-clock per update around a device synchronise.  Gate: (b) < (a) in every round,
for every method that has arm (a).

    python tools/bench_optim.py [--methods Adam,Adagrad] [--out profiles/optim_fused_ab.txt]

``--clip`` times gradient clipping instead (default ``--out profiles/clip_fused_ab.txt``): momentum
SGD and Adam over the same arena with no clipping, a constant clamp, an L2-norm threshold and both,
each as the LocalOptimizer runs it —

  (p) processors  ``bigdl.clip.fused=false``: ``run_processors`` over the gradient (Σg² by torch, a
                  clamp pass, a scaling pass), then the unclipped update kernel
  (f) fused       one ``grad_sumsq`` launch pair when an L2 threshold is set, then the update kernel
                  with the clip operand

— and the ``grad_sumsq`` launch alone, fp32 and bf16, next to a device copy of the same tensor.
Gate: median(p) - median(f) > max(p) - min(p), the processor arm's round-to-round spread, for every
clip setting.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "bigdl-1_amd"))

RESNET50_PARAMS = 25_557_032


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=RESNET50_PARAMS)
    ap.add_argument("--methods", default="", help="comma-separated subset of the methods (default: all)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--clip", action="store_true", help="time gradient clipping: fused against the processors")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(_ROOT, "profiles", "clip_fused_ab.txt" if a.clip else "optim_fused_ab.txt")

    import torch
    if not torch.cuda.is_available():
        print("bench_optim needs a GPU", file=sys.stderr)
        return 2
    from bigdl import ops
    from bigdl import optim as O
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    assert ops.native_status()["loaded"], ops.native_status()

    n = a.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad = torch.randn(n, device="cuda", generator=gen) * 1e-3
    w0 = torch.randn(n, device="cuda", generator=gen) * 0.05
    loss = torch.zeros((), device="cuda")
    if a.clip:
        return clip_ab(a, n, grad, w0, loss)
    # name -> (constructor, native op, bytes per element, has a torch arm under bigdl.optim.fused=false)
    makers = {
        "RMSprop": (lambda: O.RMSprop(learningrate=0.01, learningrate_decay=0.001), "rmsprop_step", 20, True),
        "Adadelta": (lambda: O.Adadelta(decayrate=0.9, epsilon=1e-6), "adadelta_step", 28, True),
        "Adamax": (lambda: O.Adamax(), "adamax_step", 28, True),
        "Ftrl": (lambda: O.Ftrl(learningrate=0.05, l1_regularization_strength=1e-4, l2_regularization_strength=1e-3,
                                l2_shrinkage_regularization_strength=1e-4), "ftrl_step", 28, True),
        "Adagrad": (lambda: O.Adagrad(learningrate=0.01, learningrate_decay=0.001, weightdecay=1e-4), "adagrad_step",
                    20, False),
        "Adam": (lambda: O.Adam(learningrate=1e-3, learningrate_decay=0.001), "adam_step", 28, False),
    }
    if a.methods:
        want = [m.strip() for m in a.methods.split(",") if m.strip()]
        unknown = [m for m in want if m not in makers]
        if unknown:
            ap.error(f"unknown methods {unknown}; choose from {list(makers)}")
        makers = {m: makers[m] for m in want}

    def arm(make, fused):
        meth = make()
        w = w0.clone()
        meth.shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")

        def run(iters):
            config.set_property("bigdl.optim.fused", fused)
            for _ in range(iters):
                meth.optimize(lambda _x: (loss, grad), w)
        return run

    w_c, buf_c = w0.clone(), torch.zeros(n, device="cuda")
    sh_c = torch.empty(n, dtype=torch.bfloat16, device="cuda")

    def sgd(iters):
        for _ in range(iters):
            ops.sgd_step(w_c, grad, buf_c, 0.1, 0.9, 0.0, 1e-4, False, False, 1.0, sh_c)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f(a.iters)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    lines = [f"Update phase of the elementwise methods: {n} arena elements (ResNet-50), bf16 shadow, "
             f"{a.iters} updates per round after {a.warmup} warm-up",
             "ms per update (host wall-clock around a device synchronise), arms alternated in one process",
             "bytes: B per element of the fused pass / 20 B of the momentum SGD pass",
             f"{'method':<9} {'round':>5} {'(a) torch':>10} {'(b) fused':>10} {'sgd':>7} {'a/b':>6} {'b/sgd':>6} "
             f"{'bytes':>6}"]
    gate = True
    try:
        for name, (make, op, nbytes, gated) in makers.items():
            assert ops.native_has(op), op
            arms = {"torch": arm(make, False)} if gated else {}
            arms.update(fused=arm(make, True), sgd=sgd)
            # warm-up, with a check that arm (b) reaches the kernel and arm (a) does not; a dispatcher
            # op (ops.adam_step) shows a refused kernel as a counted fallback instead
            real, seen = getattr(ops.native_ops, op), []
            setattr(ops.native_ops, op, lambda *p, **k: seen.append(real(*p, **k)) or seen[-1])
            ops.reset_fallbacks()
            try:
                if gated:
                    arms["torch"](a.warmup)
                    assert not seen, f"{op}: the torch arm called the kernel"
                arms["fused"](a.warmup)
                if op in ops.__all__:
                    assert not [k for k in ops.fallback_counts() if k[0] == op], ops.fallback_counts()
                else:
                    assert len(seen) == a.warmup and all(s is not NotImplemented for s in seen), f"{op} refused"
            finally:
                setattr(ops.native_ops, op, real)
            sgd(a.warmup)
            torch.cuda.synchronize()
            for r in range(a.rounds):
                row = {k: timed(f) for k, f in arms.items()}
                ta, ab = "-", "-"
                if gated:
                    gate = gate and row["fused"] < row["torch"]
                    ta, ab = f"{row['torch']:.3f}", f"{row['torch'] / row['fused']:.2f}"
                lines.append(f"{name:<9} {r:>5} {ta:>10} {row['fused']:>10.3f} {row['sgd']:>7.3f} "
                             f"{ab:>6} {row['fused'] / row['sgd']:>6.2f} {nbytes / 20:>6.2f}")
            del arms
            torch.cuda.empty_cache()
    finally:
        config.clear_property("bigdl.optim.fused")
    lines.append(f"gate (b) < (a) in every round, for every method with arm (a): {'PASS' if gate else 'FAIL'}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if gate else 1


def clip_ab(a, n, grad, w0, loss) -> int:
    import statistics
    import torch
    from bigdl import ops
    from bigdl import optim as O
    from bigdl.parameters import GradClip, run_processors
    assert ops.native_has("grad_sumsq") and ops.native_has("sgd_step") and ops.native_has("adam_step")
    norm = float(grad.double().square().sum().sqrt())
    # an L2 threshold the gradient exceeds, bounds that clamp about a third of the elements
    settings = {"none": (None, None), "clamp": ((-1e-3, 1e-3), None), "l2": (None, 0.5 * norm),
                "both": ((-1e-3, 1e-3), 0.5 * norm)}
    makers = {"SGD": lambda: O.SGD(learningrate=0.1, momentum=0.9, dampening=0.0, weightdecay=1e-4),
              "Adam": lambda: O.Adam(learningrate=1e-3, learningrate_decay=0.001)}

    def arm(make, const, l2, fused):
        meth = make()
        w, g = w0.clone(), grad.clone()  # the processors write the gradient: every arm owns one
        meth.shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        clip = GradClip.of(const, l2)
        procs = clip.processors() if clip is not None else []

        def run(iters):
            for _ in range(iters):
                if clip is not None and fused:
                    clip.collect(g)
                    meth.grad_clip = clip
                elif clip is not None:
                    run_processors(procs, None, g)
                meth.optimize(lambda _x: (loss, g), w)
        return run

    def timed(f, iters=a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f(iters)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    lines = [f"Gradient clipping in the update phase: {n} arena elements (ResNet-50), bf16 shadow, {a.iters} updates "
             f"per round after {a.warmup} warm-up, {a.rounds} rounds",
             "ms per update (host wall-clock around a device synchronise), arms alternated in one process",
             "(p) processors = bigdl.clip.fused=false (run_processors, then the unclipped kernel); (f) fused = "
             "grad_sumsq (L2 only) + the update kernel with the clip operand",
             f"{'method':<6} {'clip':<6} {'round':>5} {'(p) procs':>10} {'(f) fused':>10} {'p/f':>6}"]
    gate = True
    summary = []
    for name, make in makers.items():
        for tag, (const, l2) in settings.items():
            arms = {"p": arm(make, const, l2, False), "f": arm(make, const, l2, True)}
            ops.reset_fallbacks()
            for f in arms.values():
                f(a.warmup)
            assert not ops.fallback_counts(), ops.fallback_counts()
            rows = {"p": [], "f": []}
            for r in range(a.rounds):
                for k, f in arms.items():
                    rows[k].append(timed(f))
                lines.append(f"{name:<6} {tag:<6} {r:>5} {rows['p'][-1]:>10.3f} {rows['f'][-1]:>10.3f} "
                             f"{rows['p'][-1] / rows['f'][-1]:>6.2f}")
            mp, mf = statistics.median(rows["p"]), statistics.median(rows["f"])
            spread = max(rows["p"]) - min(rows["p"])
            ok = tag == "none" or mp - mf > spread
            gate = gate and ok
            summary.append(f"{name:<6} {tag:<6} median p {mp:.3f}  f {mf:.3f}  p-f {mp - mf:+.3f}  spread(p) {spread:.3f}  "
                           + ("(same path: not gated)" if tag == "none" else ("PASS" if ok else "FAIL")))
            del arms
            torch.cuda.empty_cache()
    lines += ["", "per setting: median over the rounds; gate p - f > spread(p)"] + summary
    # the reduction alone, next to a device copy of the same tensor
    lines += ["", f"grad_sumsq alone ({a.iters} launches per round, ms per launch pair) and torch copy_ of the same "
              "tensor into a buffer of its own",
              f"{'gradient':<9} {'round':>5} {'grad_sumsq':>11} {'copy_':>8} {'GB/s read':>10}"]
    out = torch.zeros(1, device="cuda")
    partials = torch.empty(ops.native_ops.SUMSQ_PARTIALS, device="cuda")
    for label, g in (("fp32", grad), ("bf16", grad.bfloat16())):
        dst = torch.empty_like(g)

        def red(iters):
            for _ in range(iters):
                ops.native_ops.grad_sumsq(g, out, partials)

        def cp(iters):
            for _ in range(iters):
                dst.copy_(g)
        red(a.warmup)
        cp(a.warmup)
        for r in range(a.rounds):
            tr, tc = timed(red), timed(cp)
            lines.append(f"{label:<9} {r:>5} {tr:>11.4f} {tc:>8.4f} {g.numel() * g.element_size() / tr / 1e6:>10.0f}")
    lines.append(f"gate: {'PASS' if gate else 'FAIL'}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main())
