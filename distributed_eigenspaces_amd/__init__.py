"""MI355X-native distributed eigenspace estimation (drop-in for TimeEscaper/distributed_eigenspaces).

Hot path (HIP, gfx950, behind the C ABI in include/deig.h):
  * sigma_hat      - covariance SYRK, split-bf16 or f32 MFMA  (distributed.py:59-70)
  * topk_eigh      - block subspace iteration + RR            (distributed.py:22-29)
  * sym_apply      - one solver sweep S Q (split-bf16 MFMA)
  * sym_power      - the solver's chain of sweeps with fused power steps
  * projavg_topk   - implicit projector-average solve         (distributed.py:126-130, NB:306)
  * topk_samples   - covariance-free worker solve: top-k straight from f32 / bf16 / uint8 rows
  * gram_apply     - its operator, alpha Xc^T (Xc Q), without a d x d matrix
  * topk_dual      - wide-data worker solve (n <= d): top-k through the n x n Gram matrix of
                     the samples, finished on topk_samples's operator
  * gram_outer     - that matrix, alpha Xc Xc^T, on the bf16 MFMA
  * procrustes_average - Procrustes-aligned basis average (one-pass aggregator, no eigensolve)
  * subspace_distance / projector_distance - residual-form sin Theta on the device
  * column_sums / sigma_hat_centered - opt-in centred covariance about a pooled mean
  * pca_transform  - fused centred scores + per-row energy and reconstruction error;
                     pca.PCA wraps the centred estimator in sklearn's conventions
  * column_sums_u8 / sigma_hat_u8_centered / pca_transform_u8 - the same centred stack on
                     uint8 samples (exact integer covariance, bytes staged by the transform;
                     PCA(k, u8_mode="raw" | "gray"))
  * sigma_hat_bf16 - bfloat16 samples as they are: one exact bf16 MFMA product, no float32
                     copy (sigma_hat dispatches to it); column_sums, sigma_hat_centered,
                     pca_transform, the estimator and PCA take bfloat16 without widening it
  * oja_step(s)    - mini-batch Oja (online variant, config 4); streaming.StreamingOja
                     adds the periodic all-gather / server solve / broadcast; bfloat16
                     batches are read as bfloat16 (two-product kernels, no float32 copy);
                     ``center=`` takes the steps about a centre on float32, bfloat16 and uint8
                     batches read in place (centred where the kernels stage a sample), and
                     StreamingOja(center=...) keeps a fixed or a running pooled mean

Drop-in modules: ``distributed`` (Node / SlaveNode / MasterNode / run_* / main),
``my_threading`` (Slave) and ``notebook`` (make_batches, top_k_eigenvectors,
compute_segma_hat, online loop).
"""
from .linalg import (EigResult, column_sums, column_sums_u8, default_subspace,  # noqa: F401
                     gram_apply, gram_outer, topk_dual, topk_samples, oja_step, oja_steps, pca_transform, pca_transform_u8, procrustes_average,
                     projavg_topk, projector_distance, sigma_hat, sigma_hat_bf16, sigma_hat_centered,
                     sigma_hat_u8_centered, stack_bases, subspace_distance, sym_apply, sym_power,
                     topk_eigh, topk_eigh_batch)
from .pca import PCA  # noqa: F401

__version__ = "0.1.0"
