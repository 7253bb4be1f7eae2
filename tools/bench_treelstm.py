"""BinaryTreeLSTM forward + backward on a GPU: the native level kernels (treelstm.hip) against the torch
level-batched path (``bigdl.treelstm.native=false``), both in one process, alternated round by round.

    python tools/bench_treelstm.py [--batch 128] [--rounds 6] [--iters 10] [--out profiles/treelstm_ab.txt]

Workload: random binary parses with 10-50 leaves padded to the batch maximum, input 300, H 150 / 250 / 256
(the TreeLSTM default, the sentiment example's default, and a multiple of 8).  Times are device events
around ``iters`` forward + backward calls after a warm-up of both paths; the host plan and the tree upload
are inside the timed region for both.
"""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))

import torch  # noqa: E402


def random_parse(n, N, rng):
    """TensorTree rows of a random binary bracketing of n leaves, padded to N nodes."""
    rows = [[0, 0, k + 1] for k in range(n)]
    spans = list(range(1, n + 1))
    while len(spans) > 1:
        k = rng.randrange(len(spans) - 1)
        rows.append([spans[k], spans[k + 1], 0])
        spans[k:k + 2] = [len(rows)]
    rows[-1][2] = -1
    return rows + [[-1, -1, -1]] * (N - len(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_treelstm needs a GPU"
    from bigdl import ops
    from bigdl.nn import BinaryTreeLSTM
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    from bigdl.utils.table import Table
    Engine.init(device="cuda:0")
    rng = random.Random(0)
    leaves = [rng.randint(10, 50) for _ in range(a.batch)]
    L, N = max(leaves), 2 * max(leaves) - 1
    trees = torch.tensor([random_parse(n, N, rng) for n in leaves], dtype=torch.float32).cuda()
    lines = [f"BinaryTreeLSTM forward + backward, B {a.batch}, leaves 10-50 (max {L}, {N} node rows), input 300, bf16; "
             f"ms per call, median [min, max] of {a.rounds} rounds x {a.iters} calls, paths alternated"]
    for H in (150, 250, 256):
        torch.manual_seed(0)
        m = BinaryTreeLSTM(300, H).to(device="cuda")
        m.training()
        x = torch.randn(a.batch, L, 300, device="cuda").to(torch.bfloat16)
        gy = torch.randn(a.batch, N, H, device="cuda").to(torch.bfloat16)
        inp = Table(x, trees)

        def run(native, k):
            config.set_property("bigdl.treelstm.native", native)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                m.forward(inp)
                m.backward(inp, gy)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / k
        ops.reset_fallbacks()
        run(True, 3)
        assert ops.fallback_counts() == {}, ops.fallback_counts()
        run(False, 3)
        t = {True: [], False: []}
        for _ in range(a.rounds):
            for native in (True, False):
                t[native].append(run(native, a.iters))
        config.set_property("bigdl.treelstm.native", True)
        ops.reset_fallbacks()
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        lines.append(f"H {H}: native {med[True]:.2f} [{min(t[True]):.2f}, {max(t[True]):.2f}]   "
                     f"torch {med[False]:.2f} [{min(t[False]):.2f}, {max(t[False]):.2f}]   x{med[False] / med[True]:.2f}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
