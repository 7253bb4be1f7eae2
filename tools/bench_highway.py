"""Highway forward + backward on a GPU: the fused MFMA gate kernels (highway.hip) against the torch matmul +
elementwise autograd path (``bigdl.highway.native=false``, the behaviour before the kernels), both in one process,
alternated round by round.

    python tools/bench_highway.py [--rounds 6] [--iters 10] [--out profiles/highway_ab.txt]

Times are device events around ``iters`` forward + backward calls after a warm-up of both arms.  Next to each
shape stands a device copy of the bytes the passes must move at least once: the bf16 weights twice (forward,
gx), the fp32 weight gradient (its store) and the six [B][N] bf16 activations and gradients.  A shape counts as
faster when the medians differ by more than the larger arm's round-to-round spread (max − min).  This is the
layer's time as a caller sees it, host plumbing and launches included; it is not a kernel time.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))

import torch  # noqa: E402

SIZES = (64, 256, 512)
BATCHES = (64, 640)


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
    assert torch.cuda.is_available(), "bench_highway needs a GPU"
    from bigdl import ops
    from bigdl.nn import Highway
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    lines = [f"Highway (tanh) forward + backward, bf16; ms per call, median [min, max] of {a.rounds} rounds x {a.iters} "
             f"calls, arms alternated; copy = device copy of 2 x W bf16 + gW fp32 + 6 x [B][N] bf16 bytes"]
    for N in SIZES:
        for B in BATCHES:
            torch.manual_seed(0)
            m = Highway(N, activation="tanh").to(device="cuda")
            m.training()
            x = torch.randn(B, N, device="cuda").to(torch.bfloat16)
            gy = torch.randn(B, N, device="cuda").to(torch.bfloat16)
            nbytes = m.weight.numel() * (2 * 2 + 4) + 6 * B * N * 2
            src, dst = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))

            def step():
                m.forward(x)
                m.backward(x, gy)

            def arm(native, k):   # the property is set outside the timed window
                config.set_property("bigdl.highway.native", native)
                return timed(step, k)
            ops.reset_fallbacks()
            arm(True, 3)
            assert ops.fallback_counts() == {}, ops.fallback_counts()
            arm(False, 3)
            timed(lambda: dst.copy_(src), 3)
            t = {True: [], False: [], "copy": []}
            for _ in range(a.rounds):
                for native in (True, False):
                    t[native].append(arm(native, a.iters))
                t["copy"].append(timed(lambda: dst.copy_(src), a.iters))
            config.set_property("bigdl.highway.native", True)
            ops.reset_fallbacks()
            med = {k_: sorted(v)[len(v) // 2] for k_, v in t.items()}
            spread = max(max(t[k_]) - min(t[k_]) for k_ in (True, False))
            ok = med[False] - med[True] > spread
            lines.append(f"B {B}, N {N}: native {med[True]:.3f} [{min(t[True]):.3f}, {max(t[True]):.3f}]   "
                         f"torch {med[False]:.3f} [{min(t[False]):.3f}, {max(t[False]):.3f}]   x{med[False] / med[True]:.2f}   "
                         f"spread {spread:.3f}   copy of {nbytes / 2 ** 20:.2f} MiB {med['copy']:.3f}   "
                         f"{'faster' if ok else 'NOT faster by more than the spread'}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
