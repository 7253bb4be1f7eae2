"""A/B of the input pipeline (one GPU): host augmentation in the native loader against the raw loader +
the device kernel (csrc/image_aug.hip), the kernel alone, and the training CLI with and without
``--deviceAugment --alterAspect``.  Arms alternate in one process, ``--rounds`` rounds each after a warm-up
of every shape.

  (a) host    NativeBatchLoader: crop / flip / normalise on the worker threads → bf16 NHWC, H2D of bf16
  (b) raw     NativeBatchLoader(raw=True): memcpy of uint8 on the workers, H2D of uint8, one kernel;
              fixed crop (the same draws as (a)) and ``alter_aspect`` + CUBIC (the reference recipe)
      both at 4 and at 16 threads, images/s over windows of at least ``--seconds`` of batches of 256
      (256² → 224²)
  (c) kernel  alone, B = 256, 256² → 224², C = 3, uint8 → bf16: staged and direct variant, CUBIC and LINEAR,
              device events over 50 launches; next to a device copy that moves the same number of bytes
              (B·H·W·C read + B·OH·OW·C·2 written) and K25 (crop / flip / normalise) at the same output size
  (d) CLI     ms/step of ``python -m bigdl.models.train.imagenet --synthetic 4096 --net resnet`` over 40
              steps, with and without the two flags, ``--cli-runs`` alternated runs each; the spread of the
              runs of one arm is printed before any difference.  The training loop does not synchronise per
              iteration (the host runs ahead until the loader's slots or the late loss read hold it), so a
              single iteration's logged time is not a step time: ms/step is the mean increment of the log's
              wall clock over iterations 11…40, leaving out the increments that span an epoch's validation

    python tools/bench_input.py [--out profiles/input_pipeline_ab.txt] [--cli-runs 3]
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "bigdl-1_amd"))

MEAN = [0.485 * 255, 0.456 * 255, 0.406 * 255]
STD = [0.229 * 255, 0.224 * 255, 0.225 * 255]


def loaders_ab(a, say):
    import numpy as np
    import torch
    from bigdl.runtime import NativeBatchLoader
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(a.images, 256, 256, 3), dtype=np.uint8)
    labels = (rng.integers(0, 1000, a.images) + 1).astype(np.float32)
    arms = {
        "host": dict(),
        "raw": dict(raw=True),
        "raw+alter": dict(raw=True, alter_aspect=(0.08, 1.0, 0.75), interp="CUBIC"),
    }
    say(f"(a)/(b) loaders: {a.images} images 256x256x3 -> 224x224 bf16 NHWC, batch 256, windows of at least "
        f"{a.seconds:g} s per arm and round, images/s")
    for threads in (4, 16):
        lds = {k: NativeBatchLoader(imgs, labels, 256, crop=(224, 224), flip=True, train=True, mean=MEAN, std=STD,
                                    dtype=torch.bfloat16, layout="NHWC", seed=1, threads=threads, prefetch=4,
                                    device="cuda", **kw) for k, kw in arms.items()}
        for ld in lds.values():  # warm-up of every arm
            for _ in range(3):
                ld.next_batch()
        torch.cuda.synchronize()
        rates = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, ld in lds.items():
                t0, nb = time.perf_counter(), 0
                while time.perf_counter() - t0 < a.seconds:
                    for _ in range(4):
                        b = ld.next_batch()
                    nb += 4
                    b.getInput().sum().item()  # the last batch has arrived
                rates[k].append(256 * nb / (time.perf_counter() - t0))
        for k in arms:
            r = rates[k]
            say(f"  threads={threads:<2} {k:<10} " + " ".join(f"{v:9.0f}" for v in r) +
                f"   median {statistics.median(r):9.0f}  spread {max(r) - min(r):7.0f}")
        for ld in lds.values():
            ld.close()


def kernel_alone(a, say):
    import torch
    from bigdl.ops import native_ops as NO
    from bigdl.ops import reference as R
    B, H, W, C, OH, OW = 256, 256, 256, 3, 224, 224
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, device="cuda", generator=gen)
    rects = torch.tensor([[0, 0, H, W]] * B)
    flip = torch.arange(B) % 2
    tab, _ = R.resample_table(src, rects, flip)
    desc = torch.from_numpy(tab).cuda()
    out = torch.empty((B, C, OH, OW), dtype=torch.bfloat16, device="cuda", memory_format=torch.channels_last)
    nbytes = B * H * W * C + B * OH * OW * C * 2
    cp_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    cp_dst = torch.empty_like(cp_src)
    oy = torch.full((B,), 16, dtype=torch.int32)
    arms = {}
    for interp in ("CUBIC", "LINEAR"):
        for variant in ("staged", "direct"):
            arms[f"{interp} {variant}"] = (lambda i=interp, v=variant: NO.image_resample_launch(
                src.reshape(-1), desc, B, C, H, W, OH, OW, MEAN, STD, False, i, torch.bfloat16, out, v))
    arms["device copy"] = lambda: cp_dst.copy_(cp_src)
    arms["K25 crop/flip/norm"] = lambda: NO.image_crop_flip_norm(src, oy, oy, flip.int(), OH, OW, MEAN, STD, False,
                                                                 torch.bfloat16)
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 50)
    say(f"(c) kernel alone: B=256 256x256x3 uint8 -> 224x224 bf16 NHWC, whole-image rectangles, {nbytes / 1e6:.1f} MB "
        f"moved, ms per launch (device events over 50 launches; K25 includes its host wrapper)")
    for k in arms:
        r = ms[k]
        say(f"  {k:<20} " + " ".join(f"{v:8.4f}" for v in r) + f"   median {statistics.median(r):8.4f}  "
            f"{nbytes / statistics.median(r) / 1e6:7.0f} GB/s of the byte count")


def cli_ab(a, say):
    base = [sys.executable, "-m", "bigdl.models.train.imagenet", "--synthetic", "4096", "--net", "resnet",
            "--maxIteration", "40", "-b", "256", "--threads", "16"]
    arms = {"host loader": [], "--deviceAugment --alterAspect": ["--deviceAugment", "--alterAspect"]}
    env = dict(os.environ, PYTHONPATH=os.path.join(_ROOT, "bigdl-1_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = {k: [] for k in arms}
    pat = re.compile(r"\[Epoch (\d+) [^\]]*\]\[Iteration (\d+)\]\[Wall Clock ([0-9.]+)s\]")
    for _ in range(a.cli_runs):
        for k, extra in arms.items():
            print(f"  [cli] {k} ...", flush=True)
            p = subprocess.run(base + extra, capture_output=True, text=True, env=env, timeout=400)
            its = [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in pat.finditer(p.stdout + p.stderr)]
            if p.returncode != 0 or len(its) < 40:
                say(f"  {k}: run failed rc={p.returncode} steps={len(its)}\n{(p.stdout + p.stderr)[-1500:]}")
                return 1
            inc = [(b[2] - a_[2]) * 1e3 for a_, b in zip(its[9:39], its[10:40]) if a_[0] == b[0]]
            res[k].append(statistics.mean(inc))
    say(f"(d) training CLI, ResNet-50 bf16, batch 256, 16 loader threads, ms/step (mean wall-clock increment of "
        f"iterations 11-40, validation gaps left out), {a.cli_runs} alternated runs")
    for k, r in res.items():
        say(f"  {k:<30} " + " ".join(f"{v:8.2f}" for v in r) + f"   median {statistics.median(r):8.2f}  "
            f"spread {max(r) - min(r):6.2f}")
    ks = list(res)
    say(f"  difference of medians {statistics.median(res[ks[1]]) - statistics.median(res[ks[0]]):+.2f} ms/step "
        f"(largest same-arm spread {max(max(r) - min(r) for r in res.values()):.2f})")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--cli-runs", type=int, default=3, help="0 skips arm (d)")
    ap.add_argument("--skip", default="", help="comma-separated arms to skip: loaders, kernel")
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "input_pipeline_ab.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_input needs a GPU", file=sys.stderr)
        return 2
    from bigdl import ops
    from bigdl.utils.engine import Engine
    Engine.init(device="cuda:0")
    assert ops.native_status()["loaded"], ops.native_status()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"Input pipeline A/B (tools/bench_input.py) on one {torch.cuda.get_device_name(0)}; {a.rounds} rounds, "
        f"arms alternated")
    rc = 0
    if "kernel" not in a.skip:
        kernel_alone(a, say)
    if "loaders" not in a.skip:
        loaders_ab(a, say)
    if a.cli_runs > 0:
        torch.cuda.synchronize()
        rc = cli_ab(a, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
