"""Parameter processors: global gradient transforms applied between the gradient all-reduce and the
optimizer update (reference ``DL/parameters/ParameterOperations.scala:33-115``,
``DL/optim/LarsSGD.scala:288-330``).

The reference runs each processor in two phases over the Spark-partitioned gradient: a
``collectGlobalData`` RDD reduce (e.g. Σg² over every partition) and a per-partition
``processParameters``.  Here a rank owns a contiguous shard of the flat fp32 gradient arena (after
the RCCL reduce-scatter), and the global reduction is one ``all_reduce`` of a small vector
(``global_sum``; identity on one process), so a processor is:

    state = {}
    for p in processors: p.collect_global_data(weight_shard, grad_shard, state, global_sum)
    for p in processors: p.process_parameters(grad_shard, state)

``Optimizer.setConstantGradientClipping`` / ``setGradientClippingByl2Norm`` install
:class:`ConstantClippingProcessor` / :class:`L2NormClippingProcessor` (``Optimizer.scala:76,
688``).  Every collective is issued by all ranks in the same order (one per processor), which keeps
RCCL's call sequence identical across ranks.

The processors are the CPU path, the path of ``LarsSGD`` and the oracle.  On the GPU, under
``bigdl.clip.fused``, the optimizers do not run them: :class:`GradClip` carries the same two
settings into the update kernels as one operand — ``ops.grad_sumsq`` takes Σg² of the raw gradient
(the bf16 wire shard included) in one deterministic pass, one float is all-reduced, and every
update kernel clips ``g·grad_scale`` right after its load, so no extra pass reads or writes the
gradient.  ``parameter_processors()`` returns the same list either way.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

GlobalSum = Callable[[torch.Tensor], torch.Tensor]


def _identity(t: torch.Tensor) -> torch.Tensor:
    return t


def sum_square(t: torch.Tensor) -> torch.Tensor:
    """Σ t² in fp32 as a 0-d tensor on t's device (``Util.getSumsquareInParallel``)."""
    return t.float().pow(2).sum()


def global_l2_norm(grad_shard: torch.Tensor, global_sum: GlobalSum = _identity) -> torch.Tensor:
    """‖g‖₂ of the whole (sharded) gradient."""
    return torch.sqrt(global_sum(sum_square(grad_shard)))


class ParameterProcessor:
    def collect_global_data(self, weight_shard: Optional[torch.Tensor], grad_shard: torch.Tensor,
                            state: Dict, global_sum: GlobalSum = _identity) -> None:
        pass

    def process_parameters(self, grad_shard: torch.Tensor, state: Dict) -> None:
        pass

    collectGlobalData = collect_global_data
    processParameters = process_parameters


class ConstantClippingProcessor(ParameterProcessor):
    """Clamp every gradient element into [min, max] (``ParameterOperations.scala:71-87``)."""

    def __init__(self, min_value: float, max_value: float):
        if min_value > max_value:
            raise ValueError(f"min {min_value} > max {max_value}")
        self.min, self.max = float(min_value), float(max_value)

    def process_parameters(self, grad_shard, state):
        grad_shard.clamp_(self.min, self.max)


class L2NormClippingProcessor(ParameterProcessor):
    """Scale the gradient by min(1, threshold / ‖g‖₂) (``ParameterOperations.scala:89-115``); the
    norm is taken over the gradient as collected, before any processor of the same step ran."""

    def __init__(self, l2_norm_threshold: float):
        if l2_norm_threshold <= 0:
            raise ValueError("l2NormThreshold must be positive")
        self.threshold = float(l2_norm_threshold)

    def collect_global_data(self, weight_shard, grad_shard, state, global_sum=_identity):
        state["l2Norm"] = global_l2_norm(grad_shard, global_sum)

    def process_parameters(self, grad_shard, state):
        norm = state["l2Norm"]
        # stays on the device (no host sync): scale = min(1, thr / ‖g‖)
        scale = torch.clamp(self.threshold / (norm + 1e-6), max=1.0)
        grad_shard.mul_(scale.to(grad_shard.dtype))


class LarsProcessor(ParameterProcessor):
    """Per-layer LARS scale (‖g_l‖ + wd·‖w_l‖) / ‖w_l‖ (``LarsSGD.scala:288-330``).

    ``parameter_splits`` maps a layer name to its (offset, length) in the flat arena;
    ``shard_range`` is the (offset, length) of this rank's shard.  The per-layer Σw², Σg² of the
    local intersection are packed into ONE vector and summed across ranks with a single collective
    (the reference's ``reduceByKey``).  Result: ``state["larsScale"][name]`` (python floats).

    Reading the scales back as Python floats synchronises the host with the device, so no optimizer
    installs this processor: the device-side equivalent is :class:`bigdl.optim.lars.LarsPlan`, which
    keeps the layer sums, the all-reduce and the per-layer rate on the device (``ops.lars_sumsq`` /
    ``ops.lars_step``) and is what the Local and Distri optimizers run for ``LarsSGD``."""

    def __init__(self, parameter_splits: Dict[str, Tuple[int, int]], weight_decay: float,
                 shard_range: Optional[Tuple[int, int]] = None):
        self.splits = dict(parameter_splits)
        self.weight_decay = float(weight_decay)
        self.shard_range = shard_range

    def collect_global_data(self, weight_shard, grad_shard, state, global_sum=_identity):
        lo, n = self.shard_range if self.shard_range is not None else (0, grad_shard.numel())
        names = sorted(self.splits)
        sums = torch.zeros(2 * len(names), dtype=torch.float32, device=grad_shard.device)
        for i, name in enumerate(names):
            off, ln = self.splits[name]
            s, e = max(lo, off), min(lo + n, off + ln)
            if e > s:
                sums[2 * i] = sum_square(weight_shard[s - lo:e - lo])
                sums[2 * i + 1] = sum_square(grad_shard[s - lo:e - lo])
        sums = global_sum(sums).tolist()
        scales = {}
        for i, name in enumerate(names):
            nw, ng = math.sqrt(sums[2 * i]), math.sqrt(sums[2 * i + 1])
            scales[name] = (ng + self.weight_decay * nw) / nw if nw > 0 else 1.0
        state["larsScale"] = scales


class GradClip:
    """Constant and L2-norm gradient clipping as ONE operand of the fused update kernels.

    ``threshold`` is the l2NormThreshold (None = no L2 clip); ``lo`` / ``hi`` the constant clamp
    (-inf / +inf = none).  With g' = g·grad_scale the clipped gradient is

        clamp(g', lo, hi) · min(1, threshold / (‖g'‖₂ + 1e-6))

    the norm taken before the clamp — what ``run_processors([ConstantClippingProcessor,
    L2NormClippingProcessor])`` does.  :meth:`apply` is that torch form; :meth:`collect` fills the
    persistent device scalar ``sumsq`` (Σg² of the RAW gradient over all ranks) that the kernels
    read, and :meth:`operands` is what a ``*_step`` wrapper hands to its kernel.  ``sumsq`` and
    ``partials`` (the reduction's scratch) are allocated once, on the first :meth:`collect`."""

    def __init__(self, threshold: Optional[float] = None, lo: float = -math.inf, hi: float = math.inf,
                 sumsq: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None):
        if threshold is not None and threshold <= 0:
            raise ValueError("l2NormThreshold must be positive")
        if lo > hi:
            raise ValueError(f"min {lo} > max {hi}")
        self.threshold = None if threshold is None else float(threshold)
        self.lo, self.hi = float(lo), float(hi)
        self.sumsq, self.partials = sumsq, partials

    @classmethod
    def of(cls, constant_clip, l2_clip) -> Optional["GradClip"]:
        """The GradClip of an optimizer's ``constant_clip`` / ``l2_clip`` settings; None for none."""
        if constant_clip is None and l2_clip is None:
            return None
        lo, hi = constant_clip if constant_clip is not None else (-math.inf, math.inf)
        return cls(l2_clip, lo, hi)

    @property
    def clamps(self) -> bool:
        return self.lo != -math.inf or self.hi != math.inf

    def processors(self) -> List[ParameterProcessor]:
        """The processor pair this object stands for, in application order."""
        procs: List[ParameterProcessor] = []
        if self.clamps:
            procs.append(ConstantClippingProcessor(self.lo, self.hi))
        if self.threshold is not None:
            procs.append(L2NormClippingProcessor(self.threshold))
        return procs

    def collect(self, grad: torch.Tensor, global_sum: GlobalSum = _identity) -> None:
        """``sumsq[0]`` = Σg² of ``grad`` (raw: not yet scaled; fp32 or the bf16 wire shard), summed
        over the ranks by ``global_sum``.  One ``grad_sumsq`` launch pair; nothing when no L2
        threshold is set."""
        if self.threshold is None:
            return
        from .. import ops
        if self.sumsq is None or self.sumsq.device != grad.device:
            self.sumsq = torch.zeros(1, dtype=torch.float32, device=grad.device)
            self.partials = torch.empty(2048, dtype=torch.float32, device=grad.device)
        ops.grad_sumsq(grad, self.sumsq, self.partials)
        total = global_sum(self.sumsq)
        if total is not self.sumsq:
            self.sumsq.copy_(total)

    def operands(self) -> Tuple[Optional[torch.Tensor], float, float, float]:
        """(sumsq or None, threshold, lo, hi) for a ``_clip`` entry point."""
        if self.threshold is None:
            return None, 0.0, self.lo, self.hi
        return self.sumsq, self.threshold, self.lo, self.hi

    def apply(self, g_scaled: torch.Tensor, grad_scale: Optional[float] = None,
              global_sum: GlobalSum = _identity) -> torch.Tensor:
        """Clip ``g_scaled`` (= g·grad_scale, fp32) in place, op for op as the two processors do.
        The norm is that of ``g_scaled`` itself, or, when ``grad_scale`` is given, the one the
        kernels use: sqrt(``sumsq``)·grad_scale from the buffer :meth:`collect` filled — the form
        for a slice of a larger gradient, whose own norm is not the global one."""
        norm = None
        if self.threshold is not None:
            if grad_scale is None:
                norm = global_l2_norm(g_scaled, global_sum)
            else:
                norm = torch.sqrt(self.sumsq.reshape(())) * float(grad_scale)
        if self.clamps:
            g_scaled.clamp_(self.lo, self.hi)
        if norm is not None:
            scale = torch.clamp(self.threshold / (norm + 1e-6), max=1.0)
            g_scaled.mul_(scale.to(g_scaled.dtype))
        return g_scaled


def run_processors(processors: Sequence[ParameterProcessor], weight_shard: Optional[torch.Tensor],
                   grad_shard: torch.Tensor, global_sum: GlobalSum = _identity) -> Dict:
    """Both phases of every processor over this rank's shard; returns the shared state table."""
    state: Dict = {}
    for p in processors:
        p.collect_global_data(weight_shard, grad_shard, state, global_sum)
    for p in processors:
        p.process_parameters(grad_shard, state)
    return state


ParameterOperations = run_processors

__all__ = ["ParameterProcessor", "ConstantClippingProcessor", "L2NormClippingProcessor", "LarsProcessor", "GradClip",
           "run_processors", "ParameterOperations", "global_l2_norm", "sum_square"]
