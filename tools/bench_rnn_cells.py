#!/usr/bin/env python
"""A/B of the native RnnCell / LSTMPeephole path (``bigdl.rnn.nativeCells``) on one GPU.

    python tools/bench_rnn_cells.py [--rounds 3] [--steps 50] [--warmup 10]

Two workloads, each a full training step (forward + criterion + backward + update through
``LocalOptimizer.train_step``) on synthetic data:

  simplernn   ``models.rnn.SimpleRNN(10000, 200, 10000)`` at B 20, T 20 (the ``models/train/rnn`` CLI's
              default batch, sequence length, hidden size and vocabulary), TimeDistributed cross-entropy
  peephole    ``Recurrent(LSTMPeephole(200, 200))`` at B 20, T 20, MSE

The arms (property true / false) alternate inside one process for ``--rounds`` rounds; each timed
region follows its own warm-up and is bracketed by device synchronisations.  Prints one line per
arm per round and a summary with the per-arm spread.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))


def _workload(name, dev):
    import torch
    from bigdl.dataset import MiniBatch
    from bigdl.nn import CrossEntropyCriterion, LSTMPeephole, MSECriterion, Recurrent, TimeDistributedCriterion
    from bigdl.optim import SGD
    from bigdl.optim.optimizer import LocalOptimizer
    B, T, H, V = 20, 20, 200, 10000
    g = torch.Generator().manual_seed(3)
    if name == "simplernn":
        from bigdl.models.rnn import SimpleRNN
        model = SimpleRNN(V, H, V)
        x = torch.randn(B, T, V, generator=g).to(dev)
        y = (torch.randint(0, V, (B, T), generator=g) + 1).float().to(dev)
        crit = TimeDistributedCriterion(CrossEntropyCriterion(), size_average=False)
    else:
        model = Recurrent().add(LSTMPeephole(H, H))
        x = torch.randn(B, T, H, generator=g).to(dev)
        y = torch.randn(B, T, H, generator=g).to(dev)
        crit = MSECriterion()
    batch = MiniBatch(x, y)
    opt = LocalOptimizer(model, [batch], crit, SGD(learningrate=0.01), batch_size=B)
    opt.prepare()
    return lambda: opt.train_step(batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    dev = Engine.device()
    for name in ("simplernn", "peephole"):
        step = _workload(name, dev)
        ms = {True: [], False: []}
        for r in range(args.rounds):
            for native in (True, False):
                config.set_property("bigdl.rnn.nativeCells", native)
                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                ms[native].append((time.perf_counter() - t0) / args.steps * 1e3)
                print(json.dumps({"workload": name, "round": r, "nativeCells": native,
                                  "ms_per_step": round(ms[native][-1], 4)}), flush=True)
        config.set_property("bigdl.rnn.nativeCells", True)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        print(json.dumps({"workload": name, "native_ms_median": round(med[True], 4),
                          "generic_ms_median": round(med[False], 4), "native_spread_ms": round(spread[True], 4),
                          "generic_spread_ms": round(spread[False], 4),
                          "difference_ms": round(med[False] - med[True], 4),
                          "ratio_generic_over_native": round(med[False] / med[True], 3)}), flush=True)


if __name__ == "__main__":
    main()
