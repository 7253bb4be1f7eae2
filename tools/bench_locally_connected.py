"""LocallyConnected2D / 1D forward + backward on a GPU: the per-location MFMA kernels (locally_connected.hip)
against the torch unfold + einsum path (``bigdl.lc.native=false``), both in one process, alternated round by
round.

    python tools/bench_locally_connected.py [--rounds 6] [--iters 10] [--out profiles/locally_connected_ab.txt]

Times are device events around ``iters`` forward + backward calls after a warm-up of both arms.  The native arm
rebuilds the data gradient's transposed weights on every call, as a training step does after its update.  Next
to each shape stands a device copy of the bytes the three passes must move at least once: the bf16 weights
(forward), the transposed bf16 weights (data gradient) and the fp32 weight gradient (its store).  A shape
counts as faster when the medians differ by more than the larger arm's round-to-round spread (max − min).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))

import torch  # noqa: E402

# (label, batch, layer constructor arguments, input shape without the batch)
SHAPES = (
    ("2-D B 64, 32->32, 32x32, k 3", 64, ("2d", 32, 32, 32, 3), (32, 32, 32)),
    ("2-D B 256, 32->32, 32x32, k 3", 256, ("2d", 32, 32, 32, 3), (32, 32, 32)),
    ("2-D B 64, 16->16, 32x32, k 9", 64, ("2d", 16, 16, 32, 9), (16, 32, 32)),
    ("1-D B 64, 128 frames x 64->64, k 5", 64, ("1d", 128, 64, 64, 5), (128, 64)),
)


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
    assert torch.cuda.is_available(), "bench_locally_connected needs a GPU"
    from bigdl import ops
    from bigdl.nn import LocallyConnected1D, LocallyConnected2D
    from bigdl.ops import native_ops as NO
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    lines = [f"LocallyConnected forward + backward, bf16; ms per call, median [min, max] of {a.rounds} rounds x "
             f"{a.iters} calls, arms alternated; copy = device copy of W bf16 + Wd bf16 + gW fp32 bytes"]
    for label, B, (kind, *c), shape in SHAPES:
        torch.manual_seed(0)
        if kind == "2d":
            cin, cout, hw, k = c
            m = LocallyConnected2D(cin, hw, hw, cout, k, k).to(device="cuda")
            x = torch.randn(B, *shape, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            wd = NO.lc_wd_numel((hw, hw, cin, cout, k, k, 1, 1, 0, 0))
        else:
            frames, cin, cout, k = c
            m = LocallyConnected1D(frames, cin, cout, k).to(device="cuda")
            x = torch.randn(B, *shape, device="cuda").to(torch.bfloat16)
            wd = NO.lc_wd_numel((1, frames, cin, cout, 1, k, 1, 1, 0, 0))
        m.training()
        gy = torch.randn_like(m.forward(x))
        nbytes = m.weight.numel() * (2 + 4) + wd * 2
        src, dst = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))

        def step(native):
            config.set_property("bigdl.lc.native", native)
            NO._LC_WD.clear()
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
        config.set_property("bigdl.lc.native", True)
        ops.reset_fallbacks()
        med = {k_: sorted(v)[len(v) // 2] for k_, v in t.items()}
        spread = max(max(t[k_]) - min(t[k_]) for k_ in (True, False))
        ok = med[False] - med[True] > spread
        lines.append(f"{label}: native {med[True]:.3f} [{min(t[True]):.3f}, {max(t[True]):.3f}]   "
                     f"torch {med[False]:.3f} [{min(t[False]):.3f}, {max(t[False]):.3f}]   x{med[False] / med[True]:.2f}   "
                     f"spread {spread:.3f}   copy of {nbytes / 2 ** 20:.1f} MiB {med['copy']:.3f}   "
                     f"{'faster' if ok else 'NOT faster by more than the spread'}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
