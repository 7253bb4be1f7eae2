"""LarsPlan: every ``LarsSGD`` of an optimizer run as one sync-free, shardable update.

The reference runs LARS on the shards: one reduce of per-layer (Σw², Σg²), then each partition
scales its own slice (``LarsSGD.scala:288-350``, installed at ``DistriOptimizer.scala:855-856``).
Here the plan owns

* a **layer table** (:class:`bigdl.ops.lars_table.LarsTable`) over the coordinate space the update
  sees — the parameter arena (LocalOptimizer, replicated mode) or this rank's shard (sharded mode,
  where a layer may have several pieces on this rank, or none);
* **one** momentum buffer over that space, the chunk partials, the ``[2L]`` layer sums and the
  ``[L, 4]`` hyper-parameter rows ``(lr·trust, weightDecay, momentum, lr)`` with a pinned host
  mirror.  The fourth column is the rate of the ``ratio = 1`` branch, which ``LarsSGD.optimize``
  takes without the trust factor.

Per step: :meth:`begin` advances every grouped method's schedule (``updateHyperParameter``, once
each, as the serial loop does), refreshes the rows with a non-blocking copy, runs ``ops.lars_sumsq``
and completes the sums with the optimizer's ``_global_sum`` (one all-reduce of 2·L floats, the
identity on one rank); :meth:`update` then runs ``ops.lars_step`` over one owned range (a bucket's
shard) or all of them.  Nothing reads the device from the host or waits for it: a staging row whose
last copy (``_RING`` steps ago) has not finished yet is replaced by a fresh pinned row.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops
from ..ops.lars_table import LarsTable

#: pinned staging rows in flight (the host may run this many steps ahead of the device)
_RING = 4


def lars_methods(optim_methods: Dict[str, object]) -> Dict[str, object]:
    """The methods of ``optim_methods`` a LarsPlan can take."""
    return {k: m for k, m in optim_methods.items() if getattr(m, "supports_layer_shards", False)}


class LarsPlan:
    def __init__(self, methods: Dict[str, object], method_slices: Dict[str, Tuple[int, int]],
                 to_space: Callable[[int, int], Sequence[Tuple[int, int, int]]], n: int, device,
                 global_sum: Callable[[torch.Tensor], torch.Tensor] = lambda t: t, chunk: int = LarsTable.CHUNK):
        """``methods``: name → LarsSGD; ``method_slices``: name → (offset, length) in the arena;
        ``to_space(lo, hi)`` maps an arena range to the parts of it this rank owns, as
        ``(space_lo, space_hi, group)`` triples (``group`` = the bucket index in sharded mode);
        ``n``: size of the space."""
        self.names = list(methods)
        self.methods = [methods[k] for k in self.names]
        self._ids = {id(m) for m in self.methods}
        self.device = torch.device(device)
        self.n = int(n)
        self._global_sum = global_sum
        pieces = []
        self._layer_method: List[int] = []     # layer → index of its method
        self._ranges: List[List[Tuple[int, int]]] = []  # method → its owned space ranges, ascending
        groups: Dict[int, List[int]] = {}
        for mi, name in enumerate(self.names):
            off, length = method_slices[name]
            owned = sorted((lo, hi) for (lo, hi, _g) in to_space(off, off + length))
            self._ranges.append(owned)
            layers = self.methods[mi].slices or [(0, length)]
            for (o, m) in layers:
                if o < 0 or m < 0 or o + m > length:
                    raise ValueError(f"LarsSGD '{name}': slice ({o}, {m}) leaves its {length} parameters")
                lid = len(self._layer_method)
                self._layer_method.append(mi)
                for (lo, hi, grp) in to_space(off + o, off + o + m):
                    pieces.append((lo, hi - lo, lid))
                    g = groups.setdefault(grp, [lo, hi])
                    g[0], g[1] = min(g[0], lo), max(g[1], hi)
        self.n_layers = len(self._layer_method)
        self.table = LarsTable(pieces, self.n_layers, self.n, self.device, chunk)
        #: group → [c0, c1) of the table (a group's chunks are contiguous: the space is group-major)
        self._group_chunks = {grp: self.table.chunk_range(lo, hi) for grp, (lo, hi) in groups.items()}
        self.v = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.sums = torch.zeros(2 * self.n_layers, dtype=torch.float32, device=self.device)
        self.hyper = torch.zeros(self.n_layers, 4, dtype=torch.float32, device=self.device)
        pin = self.device.type == "cuda"
        self._host = [torch.zeros(self.n_layers, 4, dtype=torch.float32, pin_memory=pin) for _ in range(_RING if pin else 1)]
        self._host_ev: List[Optional[torch.cuda.Event]] = [None] * len(self._host)
        self._slot = 0
        self._reduced = self.sums
        self.import_state()

    def covers(self, meth) -> bool:
        return id(meth) in self._ids

    # ------------------------------------------------------------------------------ per step
    def _refresh_hyper(self):
        slot = self._slot
        self._slot = (slot + 1) % len(self._host)
        ev = self._host_ev[slot]
        if ev is not None and not ev.query():
            # the copy that last read this row (_RING steps ago) is still in flight: stage in a fresh
            # pinned row instead of waiting (the host allocator keeps the old one until that copy ends)
            self._host[slot] = torch.zeros(self.n_layers, 4, dtype=torch.float32, pin_memory=True)
        rows = []
        for mi in self._layer_method:
            m = self.methods[mi]
            lr = -m.learningRateSchedule.currentRate
            rows.append((lr * m.trust, m.weightDecay, m.momentum, lr))
        host = self._host[slot]
        host.copy_(torch.tensor(rows, dtype=torch.float32).reshape(self.n_layers, 4))
        if self.device.type == "cuda":
            self.hyper.copy_(host, non_blocking=True)
            ev = self._host_ev[slot] or torch.cuda.Event()
            ev.record()
            self._host_ev[slot] = ev
        else:
            self.hyper.copy_(host)

    def begin(self, w: torch.Tensor, g: torch.Tensor):
        """Advance the schedules and form the layer sums of (``w``, ``g``) over the space (``g``:
        fp32, or the bf16 wire shard); every reduced gradient must already be in ``g``."""
        for m in self.methods:
            m.updateHyperParameter()
        self._refresh_hyper()
        ops.lars_sumsq(w, g, self.table, self.sums)
        self._reduced = self._global_sum(self.sums)

    def update(self, w: torch.Tensor, g: torch.Tensor, shadow: Optional[torch.Tensor], grad_scale: float,
               group: Optional[int] = None):
        """Update the owned range of ``group`` (every range when None).  ``grad_scale`` is passed
        to the kernel, not pre-multiplied."""
        if group is None:
            c0, c1 = 0, self.table.n_chunks
        elif group in self._group_chunks:
            c0, c1 = self._group_chunks[group]
        else:
            return
        if c1 > c0:
            ops.lars_step(w, g, self.v, self.table, self._reduced, self.hyper, grad_scale, shadow, c0, c1)

    # ------------------------------------------------------------------------------ checkpoints
    def export_state(self):
        """Each method's pieces of the momentum buffer, concatenated in range order, become its
        ``state["dfdx"]`` (what the checkpoint writers serialise)."""
        for m, owned in zip(self.methods, self._ranges):
            parts = [self.v[lo:hi] for lo, hi in owned]
            m.state["dfdx"] = torch.cat(parts) if parts else torch.zeros(0, device=self.device)

    def release_state(self):
        """Drop the exported copies once the checkpoint writers have taken their snapshot (the
        momentum lives in the plan's buffer; a copy left behind would double it and go stale)."""
        for m in self.methods:
            m.state.pop("dfdx", None)

    def import_state(self):
        """The inverse of :meth:`export_state`, for every method that arrives with a ``dfdx`` of
        the length of its owned ranges (a restored checkpoint, or the serial loop's buffer)."""
        for m, owned in zip(self.methods, self._ranges):
            t = m.state.get("dfdx")
            total = sum(hi - lo for lo, hi in owned)
            if not isinstance(t, torch.Tensor) or t.numel() != total or total == 0:
                continue
            t = t.reshape(-1).to(device=self.device, dtype=torch.float32)
            o = 0
            for lo, hi in owned:
                self.v[lo:hi].copy_(t[o:o + hi - lo])
                o += hi - lo
            del m.state["dfdx"]  # consumed: the momentum lives in the plan's buffer
