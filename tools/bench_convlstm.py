#!/usr/bin/env python
"""A/B of the native ConvLSTMPeephole path (``bigdl.rnn.nativeConvLSTM``) on one GPU.

    python tools/bench_convlstm.py [--rounds 3] [--steps 10] [--warmup 3] [--out profiles/convlstm_ab.txt]

The training step (forward + backward) of ``Recurrent(ConvLSTMPeephole(64, 64, 3, kC))`` at B 8, T 10, 64×64,
for kC 3 and kC 5.  The arms (property true / false) alternate inside one process for ``--rounds`` rounds;
each timed region follows its own warm-up and is timed with device events.  Also prints the bytes one
recurrent step must move (gx read, h read and written, the training saves written) and the time of a device
copy of that many bytes as the floor of one step launch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bigdl-1_amd"))


def _timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bigdl.nn import ConvLSTMPeephole, Recurrent
    from bigdl.utils import config
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    B, T, C, H, W = 8, 10, 64, 64, 64
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, C, H, W, generator=g).cuda()
    gy = torch.randn(B, T, C, H, W, generator=g).cuda()
    # per recurrent step: gx (4C bf16) read, h (C bf16) read and written, c, tanh c (C fp32) and the four
    # activations (4C fp32) written, c_{t-1} read
    step_bytes = B * H * W * C * (4 * 2 + 2 * 2 + 2 * 4 + 4 * 4 + 4)
    # a copy reads and writes: half the bytes each way; eight buffer pairs in rotation (more than the
    # 256 MB last-level cache) so that the copy runs from HBM as a step's operands do
    bufs = [torch.zeros(2, step_bytes // 2, dtype=torch.uint8, device="cuda") for _ in range(8)]
    it = iter(range(10 ** 9))

    def copy():
        b = bufs[next(it) % len(bufs)]
        b[1].copy_(b[0])

    for _ in range(8):
        copy()
    torch.cuda.synchronize()
    emit({"step_bytes": step_bytes, "copy_floor_ms": round(_timed(copy, 40), 4)})
    for kC in (3, 5):
        torch.manual_seed(0)
        model = Recurrent().add(ConvLSTMPeephole(C, C, 3, kC)).to(device="cuda")
        model.training()

        def step():
            model.forward(x)
            model.zeroGradParameters()
            model.backward(x, gy)

        ms = {True: [], False: []}
        for r in range(args.rounds):
            for native in (True, False):
                config.set_property("bigdl.rnn.nativeConvLSTM", native)
                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                ms[native].append(_timed(step, args.steps))
                emit({"kC": kC, "round": r, "nativeConvLSTM": native, "path": "convlstm" if native else "generic",
                      "ms_per_step": round(ms[native][-1], 3)})
        config.set_property("bigdl.rnn.nativeConvLSTM", True)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        emit({"kC": kC, "shape": [B, T, C, H, W], "native_ms_median": round(med[True], 3),
              "generic_ms_median": round(med[False], 3), "native_spread_ms": round(spread[True], 3),
              "generic_spread_ms": round(spread[False], 3), "difference_ms": round(med[False] - med[True], 3),
              "ratio_generic_over_native": round(med[False] / med[True], 3)})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
