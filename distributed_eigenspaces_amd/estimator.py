"""One-shot distributed eigenspace estimator across GPUs (one process per GPU).

The reference distributes shards through a RabbitMQ work queue
(distributed.py:96-143): M contiguous shards of N // M rows (remainder dropped,
:99-104), each worker returns its d x k basis as JSON, the master averages the
projectors (:126-130).  Here:

* shards: the same contiguous split; rank r owns global shards
  [r * W, (r + 1) * W) for W = workers_per_rank logical workers (they run back to
  back on the rank's GPU - each SYRK fills the chip);
* exchange: ONE collective - an all-gather of the fp32 bases (k x d rows each,
  i.e. the column-major d x k bytes) over RCCL/xGMI into Wt = [V_1^T; ...; V_M^T];
* server: the implicit projector-average top-k on ``server_rank`` (GPU 0),
  warm-started from V_1; the d x d average is never formed.  With
  ``aggregate="procrustes"`` the server is the Procrustes-aligned average instead
  (``linalg.procrustes_average``: no eigensolve, columns follow V_1's).

``center=True`` (opt-in; the reference never centres) estimates the eigenspace of the
CENTRED covariance: one more collective before the workers run - an all-reduce of the
float64 column sums and row counts into the pooled mean (``global_mean``) - and every
logical worker's covariance is taken about that pooled mean
(``linalg.sigma_hat_centered``), so the shards estimate the same matrix.  With
``u8_mode="raw"`` or ``"gray"`` (opt-in as well) uint8 samples go through that path as bytes:
the column sums are the integer ones of ``linalg.column_sums_u8`` and every worker's
covariance is ``linalg.sigma_hat_u8_centered`` about the pooled mean - the exact int8-MFMA
pipeline with centred epilogues, no widening of the shard.  The features are v = x ("raw":
one byte each) or v = (r + g + b) / 3 of interleaved pixels ("gray": (n, H, W, 3) or rows of
3-byte pixels), and ``EstimatorResult.mean`` is in units of v.  Without ``u8_mode`` uint8
samples are widened to float64 as before.

bfloat16 samples (a tensor on the device) stay bfloat16 with either setting of ``center``:
the workers' covariance is ``linalg.sigma_hat``'s bf16 kernel (one exact MFMA product, no
float32 copy) or, centred, ``linalg.sigma_hat_centered`` reading bf16, and the column sums of
the pooled mean read bf16 too.

``covariance="free"`` (opt-in; the default ``"explicit"`` is everything above, unchanged) is
the covariance-free worker route: every logical worker is ``linalg.topk_samples`` on its
shard - the top-k of X_i^T X_i / n_i straight from the float32, bfloat16 or uint8 (raw bytes)
rows, about the pooled mean with ``center=True`` - and no d x d covariance is ever formed.
It is the route for shards with far fewer rows than features and for d beyond the covariance
kernels; at tall shards it is slower than the explicit route.  Its workers run in the serial
worker loop: ``batched_workers`` and ``concurrent_workers`` do not apply and are ignored.
uint8 shards go through as raw bytes, uncentred or with ``center=True, u8_mode="raw"``;
``u8_mode="gray"`` and float64 samples are not supported by this route.  The operator is
implicit, so the solver does not deflate a dominant mean direction: uncentred data with a
large mean should use ``center=True`` or the explicit route.

``covariance="dual"`` (opt-in) is the wide-data worker route: every logical worker is
``linalg.topk_dual`` on its shard - the n_i x n_i sample-space Gram matrix on the bf16 MFMA,
its top-k, a back-projection and a finish on the same implicit operator as ``"free"``.  It is
meant for shards with n_i <= d and needs n_i <= 32768 and k <= n_i.  Everything else is as for
``"free"``: the serial worker loop, the same centring and pooled-mean plumbing, float32,
bfloat16 or raw uint8 samples, no ``u8_mode="gray"``, no float64.  No automatic choice
between the routes is made.

The collective layer only uses ``torch.distributed`` with tensors on the rank's
device, so it runs on ``gloo`` with CPU tensors too (multi-process tests); the
per-worker compute is injectable for those tests and defaults to the GPU ops.
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass

import torch
import torch.distributed as dist

from . import linalg

__all__ = ["shard_ranges", "rank_shards", "EstimatorResult", "DistributedEigenspaceEstimator",
           "gather_bases", "global_mean"]


AGGREGATES = ("projector", "procrustes")
COVARIANCES = ("explicit", "free", "dual")


def shard_ranges(n_rows: int, batches_number: int):
    """distributed.py:99-104: M contiguous (lo, hi) ranges of N // M rows."""
    step = n_rows // batches_number
    return [(i * step, (i + 1) * step) for i in range(batches_number)]


def rank_shards(n_rows: int, world: int, rank: int, workers_per_rank: int = 1):
    """The global shard ranges owned by ``rank`` (contiguous block of shards)."""
    allr = shard_ranges(n_rows, world * workers_per_rank)
    return allr[rank * workers_per_rank:(rank + 1) * workers_per_rank]


def comm_tensor(t: torch.Tensor, group=None) -> torch.Tensor:
    """The tensor the process group's backend moves for ``t``: ``t`` itself (RCCL
    moves device tensors over xGMI; gloo moves host tensors), or a host copy of a
    device tensor under gloo (the multi-rank rehearsal, several ranks sharing one
    GPU).  The collective calls are the same on both backends; only this staging
    differs."""
    if t.is_cuda and dist.get_backend(group) != "nccl":
        return t.cpu()
    return t


def gather_bases(Wt_local: torch.Tensor, group=None) -> torch.Tensor:
    """All-gather the per-rank stacks of bases ((W k) x d each) in rank order: ONE
    ``all_gather_into_tensor`` (ncclAllGather under RCCL) into Wt = [V_1^T; ...; V_M^T]."""
    if not dist.is_available() or not dist.is_initialized():
        return Wt_local
    world = dist.get_world_size(group)
    if world == 1:
        return Wt_local
    src = comm_tensor(Wt_local.contiguous(), group)
    out = torch.empty((world * src.shape[0], src.shape[1]), dtype=src.dtype, device=src.device)
    dist.all_gather_into_tensor(out, src, group=group)
    return out.to(Wt_local.device)


def global_mean(sums: torch.Tensor, n_rows: int, group=None) -> torch.Tensor:
    """Pooled column mean of all ranks' rows: ONE ``all_reduce(SUM)`` of the float64 vector
    [sums, n_rows] (this rank's column sums and row count), then sums / n.  Returns a (d,)
    float64 tensor on ``sums``' device, the same on every rank."""
    v = torch.cat([sums.detach().to(torch.float64).reshape(-1),
                   torch.tensor([float(n_rows)], dtype=torch.float64, device=sums.device)])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        buf = comm_tensor(v, group)  # v itself under RCCL, a host copy under gloo
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        v = buf.to(sums.device)
    return v[:-1] / v[-1]


@dataclass
class EstimatorResult:
    evals: torch.Tensor | None     # (k,) ascending, server rank only
    V: torch.Tensor | None         # (d, k) column-major, server rank only
    Wt: torch.Tensor               # gathered bases ((M k) x d)
    worker_evals: list             # this rank's workers' eigenvalues
    sweeps_worker: list
    sweeps_server: int
    cosines: torch.Tensor | None = None  # aggregate="procrustes": (m, k) cosines basis i / V_1
    mean: torch.Tensor | None = None     # center=True: the pooled column mean, (d,) float64


def _batch_accepts(solver_kw: dict) -> bool:
    """The batched worker solve takes these solver options (topk_eigh_batch has no
    per-problem warm start q0, for one): others fall back to the serial worker loop,
    which passes them to topk_eigh as before."""
    params = inspect.signature(linalg.topk_eigh_batch).parameters
    return all(key in params and key not in ("Ss", "k") for key in solver_kw)


def _covariance(x: torch.Tensor, center=None, u8_mode=None) -> torch.Tensor:
    """A logical worker's covariance: the reference's uncentred one, or (center=True fits)
    the covariance about the pooled mean - of the bytes themselves with ``u8_mode``."""
    if center is None:
        return linalg.sigma_hat(x)
    if u8_mode is not None:
        return linalg.sigma_hat_u8_centered(x, center=center, mode=u8_mode)
    return linalg.sigma_hat_centered(x, center=center)


def _gpu_worker(x: torch.Tensor, k: int, center=None, u8_mode=None, **kw):
    S = _covariance(x, center, u8_mode)
    r = linalg.topk_eigh(S, k, check_finite=False, **kw)
    return r.V, r.evals, r.sweeps


def _gpu_worker_free(x: torch.Tensor, k: int, center=None, u8_mode=None, **kw):
    """The covariance-free worker: top-k straight from the shard's rows (uint8: raw bytes)."""
    r = linalg.topk_samples(x, k, center=center, **kw)
    return r.V, r.evals, r.sweeps


def _gpu_worker_dual(x: torch.Tensor, k: int, center=None, u8_mode=None, **kw):
    """The wide-data worker: top-k through the shard's n x n Gram matrix (uint8: raw bytes)."""
    r = linalg.topk_dual(x, k, center=center, **kw)
    return r.V, r.evals, r.sweeps


class DistributedEigenspaceEstimator:
    def __init__(self, k: int, workers_per_rank: int = 1, server_rank: int = 0, group=None,
                 worker_fn=None, solver_kw=None, concurrent_workers: bool = False,
                 batched_workers: bool = True, aggregate: str = "projector",
                 center: bool = False, u8_mode: str | None = None, covariance: str = "explicit"):
        if aggregate not in AGGREGATES:
            raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
        if covariance not in COVARIANCES:
            raise ValueError(f"covariance must be one of {COVARIANCES}, got {covariance!r}")
        if covariance != "explicit" and u8_mode == "gray":
            raise ValueError(f"covariance={covariance!r} reads uint8 samples as raw bytes only: "
                             "u8_mode='gray' needs covariance='explicit'")
        # "explicit" (default): sigma_hat* + topk_eigh per worker; "free": linalg.topk_samples
        # on the shard's rows, no d x d covariance, serial worker loop; "dual": linalg.topk_dual
        # on them, the same loop.
        self.covariance = covariance
        free = covariance != "explicit"
        # "projector" (default, the reference's server): top-k of the projector average;
        # "procrustes": Procrustes-aligned average of the bases, reference V_1.
        self.aggregator = aggregate
        self.k = int(k)
        self.wpr = int(workers_per_rank)
        # concurrent_workers (default GPU worker, W > 1): covariances back to back on
        # the caller's stream, each worker's eigensolve in a my_threading.Slave
        # thread on its own HIP stream, chained by an event (bench.py's c5 mode).
        self.concurrent = bool(concurrent_workers) and worker_fn is None and not free
        # batched_workers (default GPU worker, W > 1, unless concurrent_workers): the W
        # covariances back to back, then ONE batched solve (linalg.topk_eigh_batch:
        # same results as W topk_eigh calls, the small Rayleigh-Ritz solves of all
        # workers in one launch per step).
        self.batched = bool(batched_workers) and worker_fn is None and not self.concurrent and not free
        self.server_rank = server_rank
        self.group = group
        self.worker_fn = worker_fn or {"free": _gpu_worker_free, "dual": _gpu_worker_dual}.get(covariance, _gpu_worker)
        self.solver_kw = dict(solver_kw or {})
        # center (opt-in): the eigenspace of the covariance about the pooled mean of all
        # ranks' rows; the default stays the reference's uncentred second moment.
        self.center = bool(center)
        # u8_mode (opt-in, center=True only): uint8 X_local is read as bytes, "raw" or "gray"
        # (linalg.sigma_hat_u8's modes); None: uint8 is widened to float64 as before.
        if u8_mode is not None and u8_mode not in ("raw", "gray"):
            raise ValueError(f"u8_mode must be None, 'raw' or 'gray', got {u8_mode!r}")
        if u8_mode is not None and not self.center:
            raise ValueError("u8_mode needs center=True (the uncentred uint8 covariance is "
                             "linalg.sigma_hat_u8)")
        self.u8_mode = u8_mode

    def _u8(self, X_local: torch.Tensor):
        """The uint8 mode this fit runs X_local in (None: the float path)."""
        return self.u8_mode if X_local.dtype == torch.uint8 else None

    def _rank_world(self):
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(self.group), dist.get_world_size(self.group)
        return 0, 1

    def pooled_mean(self, X_local: torch.Tensor) -> torch.Tensor:
        """The mean of the rows that the workers of all ranks use: this rank's
        wpr * (n // wpr) rows (the remainder is dropped, as the shards drop it)."""
        used = self.wpr * (X_local.shape[0] // self.wpr)
        rows = X_local[:used]
        # host tensors: the gloo rehearsal with an injected worker
        if self._u8(X_local) is not None:
            sums = linalg.column_sums_u8(rows, self.u8_mode)
        else:
            sums = linalg.column_sums(rows) if rows.is_cuda else rows.to(torch.float64).sum(dim=0)
        return global_mean(sums, used, self.group)

    def local_bases(self, X_local: torch.Tensor, center: torch.Tensor | None = None):
        """Run this rank's logical workers on contiguous pieces of X_local (center: the
        pooled mean of a centred fit, None = uncentred)."""
        parts = shard_ranges(X_local.shape[0], self.wpr)
        ckw = {} if center is None else {"center": center}
        u8 = self._u8(X_local) if center is not None else None
        if u8 is not None:
            ckw["u8_mode"] = u8
        if self.concurrent and len(parts) > 1 and X_local.is_cuda:
            return self._local_bases_concurrent(X_local, parts, center, u8)
        if self.batched and len(parts) > 1 and X_local.is_cuda and _batch_accepts(self.solver_kw):
            Ss = [_covariance(X_local[lo:hi], center, u8) for lo, hi in parts]
            rs = linalg.topk_eigh_batch(Ss, self.k, check_finite=False, **self.solver_kw)
            return (torch.cat([r.V.t() for r in rs], dim=0).contiguous(), [r.evals for r in rs],
                    [r.sweeps for r in rs])
        rows, evs, sw = [], [], []
        for lo, hi in parts:
            V, ev, s = self.worker_fn(X_local[lo:hi], self.k, **ckw, **self.solver_kw)
            rows.append(V.t())  # k x d view of the column-major basis
            evs.append(ev)
            sw.append(s)
        return torch.cat(rows, dim=0).contiguous(), evs, sw

    def _local_bases_concurrent(self, X_local: torch.Tensor, parts, center=None, u8=None):
        from .my_threading import Slave
        dev = X_local.device
        main = torch.cuda.current_stream(dev)
        slaves = []
        try:
            for lo, hi in parts:
                S = _covariance(X_local[lo:hi], center, u8)
                ev = torch.cuda.Event()
                ev.record(main)
                st = torch.cuda.Stream(dev)
                S.record_stream(st)

                def solve(S=S, ev=ev, st=st):
                    with torch.cuda.stream(st):
                        st.wait_event(ev)
                        r = linalg.topk_eigh(S, self.k, check_finite=False, **self.solver_kw)
                        st.synchronize()
                    return r

                sl = Slave(solve)
                sl.start()
                slaves.append((sl, st))
        finally:
            # every started solve is joined before anything propagates (no orphaned
            # threads still launching on their streams)
            for sl, _ in slaves:
                sl.join()
        errors = [sl.exception for sl, _ in slaves if sl.exception is not None]
        if errors:
            raise errors[0]
        rows, evs, sw = [], [], []
        for sl, st in slaves:
            main.wait_stream(st)
            r = sl.result
            # both outputs were allocated on the side stream; the main stream reads them
            r.V.record_stream(main)
            r.evals.record_stream(main)
            rows.append(r.V.t())
            evs.append(r.evals)
            sw.append(r.sweeps)
        return torch.cat(rows, dim=0).contiguous(), evs, sw

    def server(self, Wt: torch.Tensor, batches_number: int):
        q0 = Wt[: self.k].t()
        return linalg.projavg_topk(Wt, self.k, 1.0 / batches_number, q0=q0, **self.solver_kw)

    def fit(self, X_local: torch.Tensor) -> EstimatorResult:
        rank, world = self._rank_world()
        mean = self.pooled_mean(X_local) if self.center else None
        Wt_local, evs, sw = self.local_bases(X_local, mean)
        Wt = gather_bases(Wt_local, self.group)
        m = world * self.wpr
        if rank == self.server_rank:
            if self.aggregator == "procrustes":
                pr = linalg.procrustes_average(Wt, self.k)
                return EstimatorResult(None, pr.V, Wt, evs, sw, 0, cosines=pr.cosines, mean=mean)
            r = self.server(Wt, m)
            return EstimatorResult(r.evals, r.V, Wt, evs, sw, r.sweeps, mean=mean)
        return EstimatorResult(None, None, Wt, evs, sw, 0, mean=mean)
