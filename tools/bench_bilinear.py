"""Bilinear forward + backward on a GPU: the fused MFMA kernels (bilinear.hip) against the torch ``F.bilinear``
autograd path (``bigdl.bilinear.native=false``), both in one process, alternated round by round.

    python tools/bench_bilinear.py [--rounds 6] [--iters 10] [--out profiles/bilinear_ab.txt]

Times are device events around ``iters`` forward + backward calls after a warm-up of both arms.  Next to each
shape stands a device copy of the bytes the passes must move at least once: the bf16 weights three times
(forward, gx1, gx2) and the fp32 weight gradient (its store).  A shape counts as faster when the medians differ
by more than the larger arm's round-to-round spread (max − min).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))

import torch  # noqa: E402

GEOMS = ((128, 128, 32), (512, 512, 8), (256, 64, 128))   # (I, J, K)
BATCHES = (64, 256)


def timed(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bilinear needs a GPU"
    from bigdl import ops
    from bigdl.nn import Bilinear
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.utils.table import Table
    Engine.init(device="cuda:0")
    lines = [f"Bilinear forward + backward, bf16; ms per call, median [min, max] of {a.rounds} rounds x {a.iters} calls, "
             f"arms alternated; copy = device copy of 3 x W bf16 + gW fp32 bytes"]
    for I, J, K in GEOMS:
        for B in BATCHES:
            torch.manual_seed(0)
            m = Bilinear(I, J, K).to(device="cuda")
            m.training()
            x = Table(torch.randn(B, I, device="cuda").to(torch.bfloat16), torch.randn(B, J, device="cuda").to(torch.bfloat16))
            gy = torch.randn(B, K, device="cuda").to(torch.bfloat16)
            nbytes = m.weight.numel() * (3 * 2 + 4)
            src, dst = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))

            def step(native):
                config.set_property("bigdl.bilinear.native", native)
                m.forward(x)
                m.backward(x, gy)
            ops.reset_fallbacks()
            timed(lambda: step(True), 3)
            assert ops.fallback_counts() == {}, ops.fallback_counts()
            timed(lambda: step(False), 3)
            timed(lambda: dst.copy_(src), 3)
            t = {True: [], False: [], "copy": []}
            for _ in range(a.rounds):
                for native in (True, False):
                    t[native].append(timed(lambda: step(native), a.iters))
                t["copy"].append(timed(lambda: dst.copy_(src), a.iters))
            config.set_property("bigdl.bilinear.native", True)
            ops.reset_fallbacks()
            med = {k_: sorted(v)[len(v) // 2] for k_, v in t.items()}
            spread = max(max(t[k_]) - min(t[k_]) for k_ in (True, False))
            ok = med[False] - med[True] > spread
            lines.append(f"B {B}, I {I}, J {J}, K {K}: native {med[True]:.3f} [{min(t[True]):.3f}, {max(t[True]):.3f}]   "
                         f"torch {med[False]:.3f} [{min(t[False]):.3f}, {max(t[False]):.3f}]   x{med[False] / med[True]:.2f}   "
                         f"spread {spread:.3f}   copy of {nbytes / 2 ** 20:.1f} MiB {med['copy']:.3f}   "
                         f"{'faster' if ok else 'NOT faster by more than the spread'}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
