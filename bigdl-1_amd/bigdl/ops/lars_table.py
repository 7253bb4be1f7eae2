"""The layer table of the LARS kernels (``csrc/lars.hip``): built once on the host, read by
``ops.lars_sumsq`` / ``ops.lars_step`` (native and reference) and owned by
:class:`bigdl.optim.lars.LarsPlan`."""
from __future__ import annotations

import torch


class LarsTable:
    """Layer table of a flat update space (the arena, or one rank's shard) for the LARS kernels.

    ``pieces`` = ``[(start, length, layer), …]``: the parts of each layer that this rank owns, in
    space coordinates (a layer may have several pieces, or none).  Every piece is cut into chunks
    of at most ``chunk`` elements, so no chunk crosses a layer boundary or leaves the owned range;
    chunks are ordered by ``start``.  Everything is range-checked here, once, on the host: the
    kernels trust the table.  Device tensors: ``cstart`` int64 [K], ``clen`` / ``clayer`` int32 [K],
    ``lptr`` int32 [L+1] and ``lchunks`` int32 [K] (the chunk ids of each layer, ascending),
    ``partials`` fp32 [2K] (the scratch of the first reduction pass)."""

    CHUNK = 8192

    def __init__(self, pieces, n_layers: int, n: int, device, chunk: int = CHUNK):
        chunk = int(chunk)
        if chunk <= 0:
            raise ValueError("LarsTable: chunk must be positive")
        pieces = sorted((int(s), int(m), int(l)) for (s, m, l) in pieces if int(m) > 0)
        end = 0
        rows = []
        for s, m, l in pieces:
            if s < end or s + m > n or not 0 <= l < n_layers:
                raise ValueError(f"LarsTable: piece ({s}, {m}, layer {l}) overlaps its neighbour or leaves the space "
                                 f"[0, {n}) / the layers [0, {n_layers})")
            end = s + m
            for o in range(0, m, chunk):
                rows.append((s + o, min(chunk, m - o), l))
        self.n, self.n_layers, self.chunk, self.device = int(n), int(n_layers), chunk, torch.device(device)
        self.n_chunks = len(rows)
        self.starts = [r[0] for r in rows]
        self.lens = [r[1] for r in rows]
        self.layers = [r[2] for r in rows]
        by_layer = sorted(range(self.n_chunks), key=lambda c: (self.layers[c], c))
        lptr = [0] * (n_layers + 1)
        for c in range(self.n_chunks):
            lptr[self.layers[c] + 1] += 1
        for l in range(n_layers):
            lptr[l + 1] += lptr[l]
        dev = self.device
        self.cstart = torch.tensor(self.starts, dtype=torch.int64).to(dev)
        self.clen = torch.tensor(self.lens, dtype=torch.int32).to(dev)
        self.clayer = torch.tensor(self.layers, dtype=torch.int32).to(dev)
        self.lptr = torch.tensor(lptr, dtype=torch.int32).to(dev)
        self.lchunks = torch.tensor(by_layer, dtype=torch.int32).to(dev)
        self.partials = torch.zeros(2 * max(self.n_chunks, 1), dtype=torch.float32, device=dev)
        self.device = self.cstart.device  # with its index ("cuda" → "cuda:0"), as tensors report it
        self._elems = {}

    def chunk_range(self, lo: int, hi: int):
        """[c0, c1) of the chunks that lie inside the space range [lo, hi)."""
        import bisect
        return bisect.bisect_left(self.starts, lo), bisect.bisect_left(self.starts, hi)

    def elements(self, c0: int = 0, c1=None):
        """(element indices, their layer ids) of chunks [c0, c1): int64 tensors on the device,
        built once per range (the torch reference ops index with them)."""
        c1 = self.n_chunks if c1 is None else c1
        e = self._elems.get((c0, c1))
        if e is None:
            idx = [torch.arange(s, s + m, dtype=torch.int64) for s, m in zip(self.starts[c0:c1], self.lens[c0:c1])]
            lay = [torch.full((m,), l, dtype=torch.int64) for m, l in zip(self.lens[c0:c1], self.layers[c0:c1])]
            z = torch.zeros(0, dtype=torch.int64)
            e = (torch.cat(idx or [z]).to(self.device), torch.cat(lay or [z]).to(self.device))
            self._elems[(c0, c1)] = e
        return e
