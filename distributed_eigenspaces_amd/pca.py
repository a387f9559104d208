"""Centred PCA on top of the distributed eigenspace estimator (sklearn's conventions).

The reference and the default estimator work on the UNCENTRED second moment (SURVEY.md
§5): on data with a non-zero mean their top basis vector is the mean direction.  ``PCA``
is the opt-in centred counterpart:

* ``fit``: the estimator with ``center=True`` (one all-reduce of the float64 column sums
  into the pooled mean, every logical worker's covariance about that mean, all-gather of
  the bases, server solve), a broadcast of the server's basis to every rank, then ONE
  fused pass over the local rows (``linalg.pca_transform``) for the Gram of the scores and
  the total energy, and one more all-reduce.  The k x k Gram is diagonalised (float64, on
  every rank from the same reduced numbers), which turns the server's basis - whose
  columns are only fixed as a span by the projector average - into the principal axes in
  descending variance, and gives ``explained_variance_``.
* ``transform`` / ``reconstruction_error``: the fused centred transform kernel.

Float32, float64 and bfloat16 samples by default (bfloat16 is read as it is by the column
sums, the centred covariance and the transform's bf16 kernel; ``mean_`` stays float64 and
``components_`` float32).  uint8 samples are opt-in through
``PCA(k, u8_mode="raw")`` (features v = x, one byte each) or ``u8_mode="gray"``
(v = (r + g + b) / 3 of (n, H, W, 3) pixels or rows of 3-byte pixels): the bytes then go
through the whole stack as bytes - integer column sums into the pooled mean, the exact
int8-MFMA covariance with centred epilogues (``linalg.sigma_hat_u8_centered``) in every
worker, and ``linalg.pca_transform_u8`` (the bytes staged and centred in the kernel) for the
second pass of ``fit``, ``transform`` and ``reconstruction_error``.  ``mean_`` and
``components_`` are in units of v; ``inverse_transform`` returns float v-space rows.
Without ``u8_mode`` uint8 samples are rejected with a ``TypeError``.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import linalg
from .estimator import COVARIANCES, DistributedEigenspaceEstimator, comm_tensor
from .streaming import broadcast_basis

__all__ = ["PCA"]


class PCA:
    """Principal components of the rows of all ranks' ``X_local``.

    Attributes after ``fit`` (sklearn.decomposition.PCA's names and conventions):
      mean_ (d,) float64 - the pooled mean of the rows used;
      components_ (k, d) float32 - principal axes as rows, DESCENDING variance
        (the solvers' bases are column-major d x k, ascending);
      explained_variance_ (k,) float64 - variance of the scores with divisor N - 1, as
        sklearn (the covariances elsewhere in this package divide by n);
      explained_variance_ratio_ (k,) float64 - over the total variance sum_j var(x_j);
      n_samples_ - N, the rows used on all ranks (each rank uses
        workers_per_rank * (n // workers_per_rank) rows, as the shards do).
    """

    def __init__(self, k: int, *, workers_per_rank: int = 1, group=None,
                 aggregate: str = "projector", solver_kw=None, u8_mode: str | None = None,
                 covariance: str = "explicit"):
        if u8_mode is not None and u8_mode not in ("raw", "gray"):
            raise ValueError(f"u8_mode must be None, 'raw' or 'gray', got {u8_mode!r}")
        if covariance not in COVARIANCES:
            raise ValueError(f"covariance must be one of {COVARIANCES}, got {covariance!r}")
        if covariance != "explicit" and u8_mode == "gray":
            raise ValueError(f"covariance={covariance!r} reads uint8 samples as raw bytes only: "
                             "u8_mode='gray' needs covariance='explicit'")
        self.u8_mode = u8_mode
        # the estimator's worker route: "explicit" covariances (default), "free"
        # (linalg.topk_samples on the rows; float32, bfloat16 and raw uint8 samples) or "dual"
        # (linalg.topk_dual on them: the n x n Gram matrix, for shards with n <= d)
        self.covariance = covariance
        self.k = int(k)
        self.wpr = int(workers_per_rank)
        self.group = group
        self.aggregate = aggregate
        self.solver_kw = dict(solver_kw or {})
        self.server_rank = 0
        self.mean_ = None
        self.components_ = None
        self.explained_variance_ = None
        self.explained_variance_ratio_ = None
        self.n_samples_ = 0

    def _samples(self, X, what: str) -> torch.Tensor:
        if not isinstance(X, torch.Tensor):
            X = torch.as_tensor(X)
        if X.dtype == torch.uint8:
            if self.u8_mode is None:
                raise TypeError(f"PCA.{what}: uint8 samples need the keyword u8_mode='raw' (one "
                                "byte per feature) or u8_mode='gray' (3-byte pixels) in PCA(...); "
                                "or convert to float32 or float64")
            if X.dim() != 2 and not (self.u8_mode == "gray" and X.dim() == 4):
                raise ValueError(f"PCA.{what}: uint8 samples must be 2-D, or (n, H, W, 3) pixels "
                                 f"with u8_mode='gray', got {tuple(X.shape)}")
            if not torch.cuda.is_available():
                raise RuntimeError(f"PCA.{what}: needs a ROCm GPU; there is no CPU fallback")
            if X.device.type != "cuda":
                X = X.to(torch.device("cuda", torch.cuda.current_device()))
            return X
        if X.dtype not in (torch.float32, torch.float64, torch.bfloat16):
            raise TypeError(f"PCA.{what}: samples must be float32, float64 or bfloat16, "
                            f"got {X.dtype}")
        if X.dim() != 2:
            raise ValueError(f"PCA.{what}: samples must be 2-D (n, d), got {tuple(X.shape)}")
        if X.dtype == torch.bfloat16:  # stays bf16 through the whole stack
            return linalg.bf16_device_tensor(X, f"PCA.{what}")
        return linalg.require_device_tensor(X, f"PCA.{what}", keep_f64=True)

    def _all_reduce(self, v: torch.Tensor) -> torch.Tensor:
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            buf = comm_tensor(v, self.group)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
            v = buf.to(v.device)
        return v

    def fit(self, X_local) -> "PCA":
        X = self._samples(X_local, "fit")
        k = self.k
        est = DistributedEigenspaceEstimator(k, workers_per_rank=self.wpr, group=self.group,
                                             server_rank=self.server_rank,
                                             aggregate=self.aggregate, solver_kw=self.solver_kw,
                                             center=True, u8_mode=self.u8_mode,
                                             covariance=self.covariance)
        r = est.fit(X)
        d = r.mean.numel()  # the features (of a gray fit: the pixels)
        Vt = torch.empty((k, d), dtype=torch.float32, device=X.device)
        if r.V is not None:
            Vt.copy_(r.V.t())
        broadcast_basis(Vt, self.server_rank, self.group)
        used = self.wpr * (X.shape[0] // self.wpr)
        Y, en = self._transform(X[:used], Vt.t(), r.mean, energy=True)
        Y64 = Y.to(torch.float64)
        stats = torch.cat([(Y64.t() @ Y64).reshape(-1), en.to(torch.float64).sum().reshape(1),
                           torch.tensor([float(used)], dtype=torch.float64, device=X.device)])
        stats = self._all_reduce(stats)
        N = int(round(float(stats[-1])))
        G = stats[:k * k].reshape(k, k)
        # Rayleigh-Ritz of the scores' Gram: the principal axes inside the estimated span
        w, Q = torch.linalg.eigh((G + G.t()) * 0.5)
        w, Q = w.flip(0), Q.flip(1)  # descending
        comp = (Q.t() @ Vt.to(torch.float64)).to(torch.float32).contiguous()
        self.mean_ = r.mean
        self.components_ = comp
        self.explained_variance_ = w / max(N - 1, 1)
        self.explained_variance_ratio_ = w / stats[k * k]
        self.n_samples_ = N
        return self

    def _transform(self, X, W, mean, **kw):
        """The fused transform of the samples' kind: bytes stay bytes (u8_mode)."""
        if X.dtype == torch.uint8:
            return linalg.pca_transform_u8(X, W, mean, self.u8_mode, **kw)
        return linalg.pca_transform(X, W, mean, **kw)

    def _fitted(self):
        if self.components_ is None:
            raise RuntimeError("PCA: call fit first")

    def transform(self, X) -> torch.Tensor:
        """Scores (X - mean_) components_^T, (n, k) float32, one fused pass over X."""
        self._fitted()
        return self._transform(self._samples(X, "transform"), self.components_.t(), self.mean_)

    def reconstruction_error(self, X) -> torch.Tensor:
        """||(x_i - mean_) - P (x_i - mean_)||^2 per row, P the projector onto the
        components (the kernel's residual: accurate to a multiple of eps ||x_i - mean_||^2)."""
        self._fitted()
        return self._transform(self._samples(X, "reconstruction_error"),
                               self.components_.t(), self.mean_, residual=True)[1]

    def inverse_transform(self, Y) -> torch.Tensor:
        """mean_ + Y components_, (n, d) float32 (plain torch.addmm: not a hot path)."""
        self._fitted()
        Y = linalg.require_device_tensor(Y, "PCA.inverse_transform")
        return torch.addmm(self.mean_.to(torch.float32), Y, self.components_)
