"""Streaming (online) estimator: mini-batch Oja per rank + periodic basis aggregation.

BASELINE.json configs[3] / north_star ("a streaming Oja / mini-batch update for
the online variant"): each rank consumes its own stream of row batches (4096 x
3072 at config 4) and updates its d x k basis with one Oja step per batch
(``linalg.oja_step``: V <- orth(V + eta/b Xb^T (Xb V))).  Every ``agg_every``
batches the ranks exchange bases exactly like the one-shot estimator: one RCCL
all-gather of the fp32 bases (estimator.gather_bases), the server rank takes the
top-k of the projector average (1/m) sum V_i V_i^T with the implicit operator
(distributed.py:126-130 + NB:306, never forming d x d), and broadcasts the result,
which every rank adopts as its next iterate (warm start).

The reference has no Oja code (parity unpinned w.r.t. the reference): the step
and the aggregation schedule are checked against the float64 restatement
``oracle.ref_cpu.oja_stream`` and the estimate by sin(theta) against the planted
subspace.

The collective layer only uses ``torch.distributed``; the per-batch update and
the server solve are injectable so the control flow runs on ``gloo`` with CPU
tensors in the multi-process tests.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import linalg
from .estimator import AGGREGATES, comm_tensor, gather_bases

__all__ = ["StreamingOja", "broadcast_basis"]


def _rank_world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def broadcast_basis(Vt: torch.Tensor, src: int, group=None) -> torch.Tensor:
    """Broadcast a contiguous k x d basis image from ``src`` (in place)."""
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return Vt
    buf = comm_tensor(Vt, group)  # Vt itself under RCCL, a host copy under gloo
    dist.broadcast(buf, src=src, group=group)
    if buf is not Vt:
        Vt.copy_(buf)
    return Vt


def _gpu_sums(X: torch.Tensor) -> torch.Tensor:
    """Float64 column sums of a batch on the device (uint8: the exact integer sums)."""
    if X.dtype == torch.uint8:
        return linalg.column_sums_u8(X, "raw")
    return linalg.column_sums(X)


def _gpu_server(Wt: torch.Tensor, k: int, scale: float, q0: torch.Tensor) -> torch.Tensor:
    return linalg.projavg_topk(Wt, k, scale, q0=q0).V


def _gpu_server_procrustes(Wt: torch.Tensor, k: int, scale: float, q0: torch.Tensor) -> torch.Tensor:
    """Procrustes-aligned average with the server rank's current basis as the
    reference: the aggregated columns stay where they were (no flips or rotations
    inside the span between aggregations)."""
    return linalg.procrustes_average(Wt, k, ref=q0).V


class StreamingOja:
    """Per-rank Oja iterate with periodic projector-average aggregation.

    V0: (d, k) float32 initial basis on the rank's device (any strides; it is
    copied into a column-major buffer).  After ``aggregate()`` every rank holds
    the server's basis, columns in ascending-eigenvalue order
    (``aggregate="projector"``, the default) or, with ``aggregate="procrustes"``, the
    Procrustes-aligned average whose columns follow the server rank's basis before
    the aggregation.  bfloat16 batches are consumed as bfloat16 (``linalg.oja_steps``:
    no float32 copy of a batch or a block; the bits of the same calls on
    ``batch.float()``).

    ``center``: None (no centring), a (d,) tensor (a fixed centre, for example
    ``PCA.mean_``) or ``"running"``: the mean of every row this estimator has been given so
    far, updated BEFORE the step from the rows of the current ``partial_fit`` batch or the
    current ``partial_fit_block`` segment.  The running mean is kept as float64 column sums
    (``sums_fn``: ``linalg.column_sums`` / ``column_sums_u8``, injectable like ``step_fn``)
    plus a row count; ``aggregate()`` all-reduces both in float64 and every rank keeps
    ``others = pooled - local`` until the next aggregation, so the centre is
    ``(local + others) / (n_local + n_others)`` and nothing is counted twice.  With a
    centre, ``step_fn`` and ``block_fn`` receive it as the keyword ``center=`` (float64,
    uint8 and bfloat16 batches read in place: ``linalg.oja_steps``); without one they are
    called as before.  ``mean_`` is the current centre (None without centring, or before
    the first row of a running mean).
    """

    def __init__(self, V0: torch.Tensor, eta: float, agg_every: int = 64, server_rank: int = 0,
                 group=None, step_fn=None, server_fn=None, block_fn=None,
                 aggregate: str = "projector", center=None, sums_fn=None):
        if aggregate not in AGGREGATES:
            raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
        self.aggregator = aggregate
        d, k = V0.shape
        self.k = int(k)
        self.V = torch.empty((k, d), dtype=torch.float32, device=V0.device).t()
        self.V.copy_(V0)
        self.eta = float(eta)
        self.agg_every = int(agg_every)
        self.server_rank = int(server_rank)
        self.group = group
        self.step_fn = step_fn or linalg.oja_step
        self.server_fn = server_fn or (_gpu_server_procrustes if aggregate == "procrustes"
                                       else _gpu_server)
        self.block_fn = block_fn or linalg.oja_steps
        self.batches_seen = 0
        self.aggregations = 0
        self.sums_fn = sums_fn or _gpu_sums
        self.running = isinstance(center, str)
        if self.running and center != "running":
            raise ValueError(f"center must be None, a (d,) tensor or 'running', got {center!r}")
        self._fixed = None
        if center is not None and not self.running:
            self._fixed = torch.as_tensor(center).to(device=V0.device, dtype=torch.float64).reshape(-1)
            if self._fixed.numel() != d:
                raise ValueError(f"center must have d = {d} entries, got {self._fixed.numel()}")
        # running mean: this rank's rows since the start, the other ranks' as of the last
        # aggregation (float64 column sums and row counts)
        self._sums = torch.zeros(d, dtype=torch.float64, device=V0.device)
        self._rows = 0
        self._other_sums = torch.zeros(d, dtype=torch.float64, device=V0.device)
        self._other_rows = 0

    @property
    def mean_(self):
        """The current centre: (d,) float64, or None (no centring; no row seen yet)."""
        if not self.running:
            return self._fixed
        n = self._rows + self._other_rows
        return (self._sums + self._other_sums) / n if n > 0 else None

    def _center_kw(self, X: torch.Tensor) -> dict:
        """The ``center=`` keyword of the step on the rows X (none without centring); a
        running mean takes the rows in first."""
        if self.running:
            self._sums += self.sums_fn(X).to(device=self._sums.device, dtype=torch.float64)
            self._rows += int(X.shape[0])
        c = self.mean_
        return {} if c is None else {"center": c}

    def partial_fit(self, Xb: torch.Tensor) -> torch.Tensor:
        """One Oja step on a row batch; aggregates every ``agg_every`` batches."""
        self.step_fn(Xb, self.V, self.eta, **self._center_kw(Xb))
        self.batches_seen += 1
        if self.agg_every > 0 and self.batches_seen % self.agg_every == 0:
            self.aggregate()
        return self.V

    def partial_fit_block(self, X: torch.Tensor, batch: int, orth_every: int = 8) -> torch.Tensor:
        """Oja steps over the consecutive row batches of X (rows beyond the last full
        batch are ignored), one ``linalg.oja_steps`` call per run of batches between
        two aggregation points; aggregates exactly where ``partial_fit`` would."""
        nb = X.shape[0] // int(batch)
        i = 0
        while i < nb:
            seg = nb - i
            if self.agg_every > 0:
                seg = min(seg, self.agg_every - self.batches_seen % self.agg_every)
            Xs = X[i * batch:(i + seg) * batch]
            self.block_fn(Xs, self.V, self.eta, batch, orth_every, **self._center_kw(Xs))
            self.batches_seen += seg
            i += seg
            if self.agg_every > 0 and self.batches_seen % self.agg_every == 0:
                self.aggregate()
        return self.V

    def aggregate(self) -> torch.Tensor:
        """All-gather the rank bases, server top-k of their projector average,
        broadcast; every rank continues from the aggregated basis."""
        rank, world = _rank_world(self.group)
        Vt = self.V.t()  # contiguous k x d image of the column-major basis
        Wt = gather_bases(Vt.contiguous(), self.group)
        if rank == self.server_rank:
            vbar = self.server_fn(Wt, self.k, 1.0 / world, self.V)
            Vt.copy_(vbar.t())
        broadcast_basis(Vt, self.server_rank, self.group)
        if self.running and world > 1:
            # pooled (sums, count) in float64; what is not this rank's own is the others'
            pooled = torch.cat([self._sums, self._sums.new_tensor([float(self._rows)])])
            buf = comm_tensor(pooled, self.group)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
            if buf is not pooled:
                pooled.copy_(buf)
            self._other_sums = pooled[:-1] - self._sums
            self._other_rows = int(round(float(pooled[-1]))) - self._rows
        self.aggregations += 1
        return self.V
