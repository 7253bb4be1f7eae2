"""A/B of LookupTableSparse on one GPU: the fused embedding-bag kernels against the torch form.

A recommendation-like input: ``--bags`` bags of ``--per-bag`` ids (dense ``n x L``, no padding) over a table of
``--n-index`` rows of ``--dim`` columns, ids drawn log-uniformly (p(id) ~ 1/id, a Zipf-like draw: the first ids are
in most bags), combiner mean, no per-id weights, no maxNorm.  Two arms over one module, alternated in one process,
``--rounds`` rounds of ``--iters`` calls each after a warm-up round, timed with device events:

  (t) torch    ``bigdl.embedding.nativeBag=false``: gather, index_add_, divide (fp32 master table)
  (n) native   csrc/embedding_bag.hip; the backward includes the stable sort of the ids every call

forward (``updateOutput``) and backward (``accGradParameters``) separately, with the table in fp32 and in bf16
compute (the native arm then reads the bf16 shadow), and as the roofline arm a device copy of
``nnz·D·sizeof(T) + n·D·4`` bytes, the traffic one direction needs.

    python tools/bench_embedding_bag.py [--out profiles/embedding_bag_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "bigdl-1_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bags", type=int, default=8192)
    ap.add_argument("--per-bag", type=int, default=32)
    ap.add_argument("--n-index", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "embedding_bag_ab.txt"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("bench_embedding_bag needs a GPU", file=sys.stderr)
        return 2
    from bigdl import ops
    from bigdl.nn import LookupTableSparse
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    assert ops.native_status()["loaded"], ops.native_status()

    n, L, D = a.bags, a.per_bag, a.dim
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = torch.rand(n, L, device="cuda", generator=gen)
    ids = torch.exp(u * torch.log(torch.tensor(float(a.n_index)))).floor().clamp_(1, a.n_index)
    gy = torch.randn(n, D, device="cuda", generator=gen)
    top = torch.bincount(ids.long().reshape(-1)).max().item()

    def timed(f):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            f()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.iters

    lines = [f"LookupTableSparse, mean: {n} bags x {L} ids (nnz {n * L}), nIndex {a.n_index}, D {D}, ids log-uniform "
             f"(the most frequent id occurs {top} times), {a.iters} calls per round after one warm-up round",
             "ms per call (device events), arms alternated in one process; copy = device copy of nnz*D*sizeof(T) + n*D*4 B",
             f"{'table':<6} {'pass':<4} {'round':>5} {'(t) torch':>10} {'(n) native':>11} {'copy':>8} {'t/n':>6} {'n/copy':>7}"]
    slower = []
    try:
        for dt, size in (("fp32", 4), ("bf16", 2)):
            config.set_property("bigdl.compute.dtype", dt)
            Engine.init(device="cuda:0")
            mod = LookupTableSparse(a.n_index, D, "mean").cuda()
            src = torch.empty(n * L * D * size + n * D * 4, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)

            def fwd(native):
                config.set_property("bigdl.embedding.nativeBag", native)
                mod.updateOutput(ids)

            def bwd(native):
                if native:
                    mod._bag_state["sort"] = None  # fresh ids every step in training: sort every call
                mod.accGradParameters(ids, gy)

            for name in ("fwd", "bwd"):
                arms = {nat: (lambda nat=nat: fwd(nat)) if name == "fwd" else (lambda nat=nat: bwd(nat))
                        for nat in (False, True)}
                ops.reset_fallbacks()
                rows = {False: [], True: [], "copy": []}
                for r in range(-1, a.rounds):  # round -1 is the warm-up
                    for native in (False, True):
                        fwd(native)  # a backward reads the state its own arm's forward left
                        assert (mod._bag_state is not None) == native
                        t = timed(arms[native])
                        if r >= 0:
                            rows[native].append(t)
                    t = timed(lambda: dst.copy_(src))
                    if r >= 0:
                        rows["copy"].append(t)
                        lines.append(f"{dt:<6} {name:<4} {r:>5} {rows[False][-1]:>10.4f} {rows[True][-1]:>11.4f} "
                                     f"{t:>8.4f} {rows[False][-1] / rows[True][-1]:>6.2f} {rows[True][-1] / t:>7.2f}")
                assert not ops.fallback_counts(), ops.fallback_counts()
                if min(rows[False]) <= max(rows[True]):
                    slower.append(f"{dt} {name}")
            del mod, src, dst
            torch.cuda.empty_cache()
    finally:
        config.clear_property("bigdl.compute.dtype")
        config.clear_property("bigdl.embedding.nativeBag")
    lines.append("cells where the native arm is not faster than the torch form in every round: "
                 + (", ".join(slower) if slower else "none"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
