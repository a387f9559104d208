"""Device-level API of the hot path: PyTorch-ROCm tensors in, HIP kernels via the C ABI.

Buffers are torch tensors on ``cuda:<i>`` (HIP under ROCm); PyTorch is used only
for device memory, streams and collectives.  Every op launches on the current
torch stream of the tensor's device and returns without a host sync, except the
eigensolvers, which synchronise that stream between sweeps to test convergence
(the reference's scipy.linalg.eigh is synchronous too).

There is no CPU fallback: inputs must live on a ROCm device, and the ops raise
if ``libdeig.so`` is missing.
"""
from __future__ import annotations

import ctypes
import threading
import warnings
from dataclasses import dataclass

import torch

from . import _lib

__all__ = [
    "sigma_hat", "topk_eigh", "topk_eigh_batch", "projavg_topk", "oja_step", "default_subspace",
    "EigResult", "require_device_tensor", "project", "stack_bases", "gemm_skinny",
    "oja_steps", "oja_check", "sym_apply", "sym_power", "sigma_hat_u8", "sigma_hat_shift",
    "procrustes_average", "subspace_distance", "projector_distance", "ProcrustesResult",
    "column_sums", "sigma_hat_centered", "pca_transform",
    "column_sums_u8", "sigma_hat_u8_centered", "pca_transform_u8",
    "sigma_hat_bf16", "bf16_device_tensor",
    "gram_apply", "topk_samples", "gram_outer", "topk_dual",
]

DEFAULT_TOL = 1e-6
DEFAULT_MAX_SWEEPS = 300
MAX_P = 128  # widest subspace of one solver block (kMaxP in csrc/solver.hip); k > 128
             # is solved in locked blocks of p - 16 pairs


class IndefiniteWarning(RuntimeWarning):
    """topk_eigh returned a negative eigenvalue: the input is not PSD."""


@dataclass
class EigResult:
    """Top-k eigenpairs, ascending order (LAPACK / scipy.linalg.eigh convention)."""

    evals: torch.Tensor   # (k,) float32
    V: torch.Tensor       # (d, k) float32, column-major (Fortran) strides (1, d)
    sweeps: int
    resid: float          # max_j ||A v_j - lambda_j v_j|| / |lambda_max|
    converged: bool


# ---------------------------------------------------------------- workspace cache
class _Workspace(threading.local):
    def __init__(self):
        self.bufs = {}


_ws = _Workspace()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _workspace(device: torch.device, nbytes: int, stream: int | None = None) -> torch.Tensor:
    """Per-thread, per-device, per-stream grow-only uint8 workspace (stream: the device's
    current stream, for a caller that has looked it up already)."""
    key = (device.index, _stream(device) if stream is None else stream)
    buf = _ws.bufs.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws.bufs[key] = buf
    return buf


def _call(device: torch.device, name: str, args: tuple, query: str, qargs: tuple) -> int:
    """The one call path of the entry points that end in ``(ws, ws_bytes, stream)``: on
    ``device``, size the workspace with ``query(*qargs)``, take this thread's cached buffer
    (never NULL; what an earlier call left in it stays when it is large enough), call
    ``name(*args, ws, ws_bytes, stream)`` on the current stream and map the return code
    (``_lib.check``).  Returns the code (DEIG_OK or DEIG_NOT_CONVERGED)."""
    L = _lib.lib()
    with torch.cuda.device(device):
        nbytes = getattr(L, query)(*qargs)
        stream = _stream(device)
        rc = getattr(L, name)(*args, _workspace(device, nbytes, stream).data_ptr(), nbytes, stream)
    return _lib.check(rc, name)


def require_device_tensor(t, name: str = "input", keep_f64: bool = False) -> torch.Tensor:
    """float32 tensor on a ROCm device (host arrays are copied over).  No CPU path.
    keep_f64: float64 input stays float64 (the reference's dtype; the covariance and
    the solver take it as is)."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            f"{name}: distributed_eigenspaces_amd runs only on a ROCm GPU (MI355X); "
            "no GPU is visible and there is no CPU fallback")
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.device.type != "cuda":
        t = t.to(device=torch.device("cuda", torch.cuda.current_device()))
    if keep_f64 and t.dtype == torch.float64:
        return t
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t


def _to_device(t: torch.Tensor, name: str) -> torch.Tensor:
    """``t`` on a ROCm device with its dtype kept (a host tensor is copied over)."""
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: needs a ROCm GPU; there is no CPU fallback")
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t


def bf16_device_tensor(t: torch.Tensor, name: str = "input") -> torch.Tensor:
    """A bfloat16 tensor on a ROCm device, kept bfloat16 (host tensors are copied over)."""
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name} needs bfloat16 samples, got {t.dtype}")
    return _to_device(t, name)


def _rowmajor(t: torch.Tensor, name: str, q: int = 4) -> torch.Tensor:
    """2-D row-major view with unit column stride, columns and row stride % q == 0 (4; 8 for
    bfloat16 samples), 16-B aligned; anything else (a 37-column slice of a 40-column tensor
    included) is copied into a zero-padded tensor of ``t``'s own dtype, so what lies behind
    the columns never enters."""
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got shape {tuple(t.shape)}")
    ok = (t.stride(1) == 1 and t.stride(0) % q == 0 and t.stride(0) >= t.shape[1]
          and t.shape[1] % q == 0 and t.data_ptr() % 16 == 0)
    return t if ok else _pad_cols(t, -(-t.shape[1] // q) * q)


def _pad_cols(t: torch.Tensor, dp: int) -> torch.Tensor:
    """A fresh contiguous copy of the 2-D ``t``, in its dtype, with its columns zero-padded to dp."""
    out = torch.zeros((t.shape[0], dp), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


# dtype -> (element-type code, elements of the narrowest load group, base alignment in bytes)
# of the samples that the packed entry points read in place (csrc/sample_src.hpp kSampleRules)
_SAMPLE_TYPES = {torch.float32: ("DEIG_F32", 4, 16), torch.bfloat16: ("DEIG_BF16", 8, 16),
                 torch.uint8: ("DEIG_U8", 4, 4)}


def _in_place(X: torch.Tensor) -> bool:
    """Can a packed entry point read the 2-D float32 / bfloat16 / uint8 X where it lies?"""
    _, q, align = _SAMPLE_TYPES[X.dtype]
    d = X.shape[1]
    ldx = _ld(X, 0, d)
    return (d >= q and d % q == 0 and X.stride(1) == 1 and ldx >= d and ldx % q == 0
            and X.data_ptr() % align == 0)


def _packed_samples(X, name: str, xname: str, dmin: int = 0):
    """``(X, xtype, n, d, dp)`` of the samples of a packed entry point (deig_oja_steps_centered,
    deig_gram_apply, deig_topk_samples): uint8 and bfloat16 samples stay what they are,
    anything else becomes float32; on the device and read where they lie when strides and
    alignment allow (``_in_place``, and d >= dmin), otherwise from a zero-padded copy of the
    SAME dtype with dp columns, dp = d rounded up to the type's load group, at least dmin."""
    if isinstance(X, torch.Tensor) and X.dtype in (torch.uint8, torch.bfloat16):
        X = _to_device(X, name)
    else:
        X = require_device_tensor(X, name)
    if X.dim() != 2:
        raise ValueError(f"{xname} must be 2-D, got shape {tuple(X.shape)}")
    n, d = X.shape
    code, q, _ = _SAMPLE_TYPES[X.dtype]
    dp = max(dmin, -(-d // q) * q)
    if dp != d or not _in_place(X):
        X = _pad_cols(X, dp)
    return X, getattr(_lib, code), n, d, dp


def _stack_4(Wt: torch.Tensor, dp: int) -> torch.Tensor:
    """The (m k) x d stack of bases as the servers read it: dp columns, unit column stride,
    row stride % 4 == 0, 16-byte aligned (a zero-padded copy where it is not)."""
    if dp != Wt.shape[1] or Wt.stride(1) != 1 or Wt.stride(0) % 4 or Wt.data_ptr() % 16:
        Wt = _pad_cols(Wt, dp)
    return Wt


def _ld(t: torch.Tensor, dim: int, extent: int) -> int:
    """Leading dimension of ``t`` along ``dim`` as the library wants it (>= extent, the
    length of one row or column).  For a dimension of size 1 torch reports an arbitrary
    stride (``(1, 1)`` for a ``(d, 1)`` tensor, whatever its layout): there is no second
    row or column, so the extent itself describes the same memory."""
    return int(extent) if t.shape[dim] == 1 else t.stride(dim)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _check_k(k, d: int) -> int:
    k = int(k)
    if not 1 <= k <= d:
        raise ValueError(f"k={k} out of range [1, {d}]")
    return k


def _elem_type(dtype: torch.dtype) -> int:
    """The library's element-type code of a float32 / float64 / bfloat16 operand."""
    if dtype == torch.bfloat16:
        return _lib.DEIG_BF16
    return _lib.DEIG_F64 if dtype == torch.float64 else _lib.DEIG_F32


def _check_result_dtype(dtype: torch.dtype) -> None:
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")


def _alpha(alpha, n: int) -> float:
    return (1.0 / n) if alpha is None else float(alpha)


def _nan_cov(d: int, dtype: torch.dtype, device, with_mean: bool = False):
    """The covariance of n = 0 samples (numpy: zeros / 0 -> NaN, with a RuntimeWarning; that
    value is kept): a (d, d) NaN tensor, with_mean: also the (d,) float64 NaN mean."""
    S = torch.full((d, d), float("nan"), dtype=dtype, device=device)
    return (S, torch.full((d,), float("nan"), dtype=torch.float64, device=device)) \
        if with_mean else S


def _cov_outputs(S: torch.Tensor, ld: int, f64_first: bool) -> tuple:
    """The two output slots of a covariance entry point, ``(S64, lds64, S, lds)`` for float
    samples (f64_first) and ``(S, lds, S64, lds64)`` for uint8 ones: ``S`` in the slot of
    its dtype, NULL in the other."""
    mine, null = (S.data_ptr(), ld), (None, ld)
    return mine + null if (S.dtype == torch.float64) == f64_first else null + mine


def default_subspace(d: int, k: int) -> int:
    return int(_lib.lib().deig_default_subspace(int(d), int(k)))


# ---------------------------------------------------------------- covariance
def sigma_hat(x: torch.Tensor, alpha: float | None = None,
              out: torch.Tensor | None = None, algo: str = "auto",
              shift: bool | None = None, dtype: torch.dtype | None = None,
              accumulate: bool = False) -> torch.Tensor:
    """Sigma_hat = alpha * X^T X with alpha = 1/n by default (uncentered).

    GPU replacement for ``SlaveNode.compute_sigma_hat_`` (distributed.py:59-70).
    x: (n, d) on the GPU (host arrays are copied over):
      * float32 (default path): a (d, d) float32 tensor, bit-exactly symmetric.
        algo: "split3" (fp32 operands as bf16 hi/lo pairs on bf16 MFMA, fp32
        accumulation, see include/deig.h), "fp32" (f32 MFMA fma chain) or "auto"
        (split3 for n >= 1024 rows, fp32 below);
      * float64 (the reference's dtype, distributed.py:171) or ``shift=True``: the
        mean-shifted covariance (deig_syrk_shift: the SYRK runs on X - mu, the mean
        terms are added in double) returned as float64 - the small eigenvectors of an
        uncentered covariance keep float64 parity (csrc/shift.hip);
      * uint8 samples: the exact integer path (sigma_hat_u8; 2-D raw bytes or
        N x H x W x 3 pixels with the reference's grayscale fused in);
      * bfloat16 samples: taken as they are (sigma_hat_bf16: one exact bf16 MFMA product,
        no float32 copy; ``accumulate`` works as for float32); with ``shift=True`` the
        mean-shifted path reads them as bf16 too.
    dtype: result dtype (float32 / float64) for the shifted and uint8 paths.
    accumulate: ``out += alpha X^T X`` (float32 split3 path; a covariance streamed
    through in row blocks, DEIG_SYRK_ACCUMULATE).
    """
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    if x.dtype == torch.uint8:
        return sigma_hat_u8(x, alpha=alpha, out=out, dtype=dtype or torch.float32)
    if x.dtype == torch.bfloat16 and not shift:
        return sigma_hat_bf16(x, alpha=alpha, out=out, accumulate=accumulate)
    if shift is None:
        shift = x.dtype == torch.float64
    if shift:
        if accumulate:
            raise ValueError("accumulate is for the float32 split3 path (shift=False)")
        return sigma_hat_shift(x, alpha=alpha, out=out, dtype=dtype or torch.float64)
    if algo not in _lib.SYRK_ALGOS:
        raise ValueError(f"algo must be one of {sorted(_lib.SYRK_ALGOS)}, got {algo!r}")
    code = _lib.SYRK_ALGOS[algo]
    x = require_device_tensor(x, "sigma_hat")
    if accumulate:
        if out is None or algo == "fp32" or x.shape[1] % 4 or not out.is_contiguous():
            raise ValueError("accumulate needs out (contiguous d x d float32), d % 4 == 0 and "
                             "the split3 algorithm")
        code = _lib.DEIG_SYRK_SPLIT3 | _lib.DEIG_SYRK_ACCUMULATE
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D (n, d), got {tuple(x.shape)}")
    n, d = x.shape
    if n == 0:
        return _nan_cov(d, torch.float32, x.device)
    xx = _rowmajor(x, "x")
    dp = xx.shape[1]
    if out is not None and dp == d and out.shape == (d, d) and out.is_contiguous() \
            and out.dtype == torch.float32 and out.device == x.device and d % 4 == 0:
        S = out
    else:
        S = torch.empty((dp, dp), dtype=torch.float32, device=x.device)
    _call(x.device, "deig_syrk_f32_ex",
          (xx.data_ptr(), n, dp, xx.stride(0), _alpha(alpha, n), S.data_ptr(), S.stride(0), code),
          "deig_syrk_workspace_ex", (n, dp, code))
    if dp != d:
        S = S[:d, :d].contiguous()
        if out is not None:
            out.copy_(S)
            return out
    return S


def sigma_hat_bf16(x: torch.Tensor, alpha: float | None = None,
                   out: torch.Tensor | None = None, accumulate: bool = False) -> torch.Tensor:
    """Sigma_hat = alpha * X^T X (alpha = 1/n by default) of bfloat16 samples, read as they
    are (include/deig.h deig_syrk_bf16): every bf16 x bf16 product is exact in float32, so
    one MFMA product per fragment pair and a two-level float32 summation - no float32 copy
    of x, no hi/lo split.  Returns a (d, d) float32 tensor, bit-exactly symmetric.
    x: (n, d) bfloat16 on the GPU (host tensors are copied over); a view that is not
    row-major with d % 8 == 0, a row stride % 8 == 0 and 16-byte alignment is copied into a
    zero-padded bfloat16 tensor.  accumulate: ``out += alpha X^T X`` (out: contiguous
    (d, d) float32, d % 8 == 0), a covariance streamed through in row blocks."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    x = bf16_device_tensor(x, "sigma_hat_bf16")
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D (n, d), got {tuple(x.shape)}")
    n, d = x.shape
    direct = (out is not None and d % 8 == 0 and out.shape == (d, d) and out.is_contiguous()
              and out.dtype == torch.float32 and out.device == x.device)
    if accumulate and not direct:
        raise ValueError("accumulate needs out (contiguous d x d float32 on x's device) and "
                         "d % 8 == 0")
    if n == 0:
        return _nan_cov(d, torch.float32, x.device)
    xx = _rowmajor(x, "x", 8)
    dp = xx.shape[1]
    S = out if direct else torch.empty((dp, dp), dtype=torch.float32, device=x.device)
    _call(x.device, "deig_syrk_bf16",
          (xx.data_ptr(), n, dp, _ld(xx, 0, dp), _alpha(alpha, n), S.data_ptr(), S.stride(0),
           _lib.DEIG_SYRK_ACCUMULATE if accumulate else 0),
          "deig_syrk_bf16_workspace", (n, dp))
    if direct:
        return out
    if dp != d:
        S = S[:d, :d].contiguous()
    if out is not None:
        out.copy_(S)
        return out
    return S


def sigma_hat_shift(x: torch.Tensor, alpha: float | None = None,
                    out: torch.Tensor | None = None,
                    dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """Mean-shifted covariance alpha * X^T X (alpha = 1/n: distributed.py:59-70) of
    float32 / float64 samples (include/deig.h deig_syrk_shift): the SYRK runs on
    C = fl32(X - mu) and the mean terms are added in double, so its rounding is
    relative to the centred data instead of the dominant mean direction of an
    uncentered covariance.  Returns a (d, d) tensor of ``dtype`` (float64: the
    reference's), bit-exactly symmetric."""
    x = _float_samples(x, "sigma_hat_shift")
    _check_result_dtype(dtype)
    n, d = x.shape
    if n == 0:
        return _nan_cov(d, dtype, x.device)
    xtype = _elem_type(x.dtype)
    S = torch.empty((d, d), dtype=dtype, device=x.device)
    _call(x.device, "deig_syrk_shift",
          (x.data_ptr(), xtype, n, d, x.stride(0), _alpha(alpha, n), *_cov_outputs(S, d, True)),
          "deig_syrk_shift_workspace", (n, d, xtype))
    if out is not None:
        out.copy_(S)
        return out
    return S


def _float_samples(x, name: str) -> torch.Tensor:
    """(n, d) float32 / float64 / bfloat16 samples on the device with unit column stride
    (bfloat16 stays bfloat16: DEIG_BF16)."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    if x.dtype == torch.bfloat16:
        x = bf16_device_tensor(x, name)
    else:
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        x = require_device_tensor(x, name, keep_f64=True)
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D (n, d), got {tuple(x.shape)}")
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def column_sums(x: torch.Tensor) -> torch.Tensor:
    """sums[j] = sum_r x[r, j] in double (include/deig.h deig_colsum): a (d,) float64
    tensor, summed in a fixed order (deterministic).  x: (n, d) float32 / float64.  The
    pooled mean of a multi-GPU centred fit is the all-reduce of these over the row count
    (``estimator.global_mean``)."""
    x = _float_samples(x, "column_sums")
    n, d = x.shape
    sums = torch.zeros(d, dtype=torch.float64, device=x.device)
    if n == 0 or d == 0:
        return sums
    _call(x.device, "deig_colsum",
          (x.data_ptr(), _elem_type(x.dtype), n, d, _ld(x, 0, d), sums.data_ptr()),
          "deig_colsum_workspace", (n, d))
    return sums


def sigma_hat_centered(x: torch.Tensor, center: torch.Tensor | None = None,
                       alpha: float | None = None, dtype: torch.dtype | None = None,
                       return_mean: bool = False):
    """Centred covariance alpha * sum_r (x_r - c)(x_r - c)^T with alpha = 1/n by default
    (include/deig.h deig_syrk_centered).  Opt-in: ``sigma_hat`` stays the reference's
    uncentred second moment.  center: (d,) float64 (the pooled mean of a multi-shard fit,
    so that the shards' covariances add up to the pooled one), None = this shard's own
    mean.  The SYRK runs on fl32(x - own mean) whatever the centre; the centre enters
    through rank-one terms in double.  Returns a (d, d) tensor of ``dtype`` (float64 by
    default), bit-exactly symmetric; with ``return_mean`` also the shard's own mean
    ((d,) float64)."""
    x = _float_samples(x, "sigma_hat_centered")
    dtype = dtype or torch.float64
    _check_result_dtype(dtype)
    n, d = x.shape
    if n == 0:
        return _nan_cov(d, dtype, x.device, return_mean)
    c = None
    if center is not None:
        c = torch.as_tensor(center).to(device=x.device, dtype=torch.float64).contiguous()
        if c.shape != (d,):
            raise ValueError(f"center must have shape ({d},), got {tuple(c.shape)}")
    xtype = _elem_type(x.dtype)
    S = torch.empty((d, d), dtype=dtype, device=x.device)
    mean = torch.empty(d, dtype=torch.float64, device=x.device) if return_mean else None
    _call(x.device, "deig_syrk_centered",
          (x.data_ptr(), xtype, n, d, _ld(x, 0, d), _ptr(c), _alpha(alpha, n),
           *_cov_outputs(S, d, True), _ptr(mean)),
          "deig_syrk_centered_workspace", (n, d, xtype))
    return (S, mean) if return_mean else S


def _u8_samples(x, mode: str, name: str):
    """The input normalisation of the uint8 ops: ``(x2, mode, n, d, dp)`` with x2 the
    samples as the library reads them - 2-D uint8 on the device, unit column stride, rows
    4-byte aligned - ``mode`` resolved ("auto": "gray" for 4-D pixels, else "raw"), d the
    number of features and dp = d rounded up to a multiple of 4.  Accepts (n, d) raw bytes,
    (n, H, W, 3) pixels and (n, 3 m) rows of 3-byte pixels with mode "gray".  Whatever does
    not meet the layout rules is copied into a zero-filled buffer of dp features: the
    padding features are zero bytes, so they add exact zeros to every sum and product."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    if x.dtype != torch.uint8:
        raise ValueError(f"{name} needs uint8 samples, got {x.dtype}")
    x = _to_device(x, name)
    if mode == "auto":
        mode = "gray" if x.dim() == 4 else "raw"
    if mode not in _lib.U8_MODES:
        raise ValueError(f"mode must be 'auto', 'raw' or 'gray', got {mode!r}")
    n = x.shape[0]
    if mode == "gray":
        if x.dim() == 4:
            if x.shape[3] != 3:
                raise ValueError(f"gray mode needs (n, H, W, 3) pixels, got {tuple(x.shape)}")
            x = x.reshape(n, -1)
        if x.dim() != 2 or x.shape[1] % 3:
            raise ValueError("gray mode needs rows of 3-byte pixels")
        d = x.shape[1] // 3
    else:
        if x.dim() != 2:
            raise ValueError(f"raw mode needs a 2-D (n, d) tensor, got {tuple(x.shape)}")
        d = x.shape[1]
    width = 3 * d if mode == "gray" else d
    dp = (d + 3) // 4 * 4
    if n > 0 and (x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 4 or dp != d):
        wp = 3 * dp if mode == "gray" else dp
        xx = torch.zeros((n, (wp + 3) // 4 * 4), dtype=torch.uint8, device=x.device)
        xx[:, :width] = x[:, :width]
        x = xx
    return x, mode, n, d, dp


def _pad_vector(v, d: int, dp: int, device, name: str):
    """(d,) float64 vector on the device with unit stride and 8-byte alignment, zero-padded to
    dp entries: a padded column stages fl32(0 - 0) = 0 (None stays None)."""
    if v is None:
        return None
    v = torch.as_tensor(v).to(device=device, dtype=torch.float64).reshape(-1)
    if v.numel() != d:
        raise ValueError(f"{name} must hold d = {d} numbers, got {v.numel()}")
    if dp != d:
        v = torch.cat([v, v.new_zeros(dp - d)])
    elif v.stride(0) != 1 or v.data_ptr() % 8:
        v = v.clone()
    return v


def _transform_operands(W, d, dp, mean, dev, wname: str, multiple: int = 4):
    """The W and mean operands of ``project`` and the PCA transforms: ``(W, mean, k)`` with
    W (checked: 2-D, 1 <= k <= 256, rows matching the samples) zero-padded to dp rows and
    column-major, mean as ``_pad_vector`` gives it on ``dev``.  d: the number of features
    when the samples fix it (uint8); None when W's rows do, the samples having dp columns
    (d itself, or d rounded up to a multiple of ``multiple``: 4 floats, 8 bfloat16).  The
    padding rows and entries are zero: they meet zero columns of the samples."""
    W = require_device_tensor(W, wname)
    if W.dim() != 2:
        raise ValueError(f"{wname} must be 2-D (d, k), got shape {tuple(W.shape)}")
    rows, k = W.shape
    if not 1 <= k <= 256:
        raise ValueError(f"k={k} out of range [1, 256]")
    if d is None:
        d = rows
        if d > dp or (dp != d and dp != -(-d // multiple) * multiple):
            raise ValueError(f"shape mismatch: X has {dp} columns, W has {d} rows")
    elif rows != d:
        raise ValueError(f"shape mismatch: X has {d} features, W has {rows} rows")
    mean = _pad_vector(mean, d, dp, dev, "mean")
    if dp != d:
        Wp = torch.zeros((dp, k), dtype=torch.float32, device=W.device)
        Wp[:d] = W
        W = Wp
    return W.t().contiguous().t(), mean, k


def _transform_buffers(n: int, k: int, dev, residual: bool, energy: bool):
    """(Y, res, en): Y (n, k) and, where asked for, the residuals and energies (n,), else None."""
    return (torch.empty((n, k), dtype=torch.float32, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev) if residual else None,
            torch.empty(n, dtype=torch.float32, device=dev) if energy else None)


def _transform_result(Y, res, en):
    """Y, or the tuple (Y[, residual][, energy])."""
    return Y if res is None and en is None else tuple(t for t in (Y, res, en) if t is not None)


def column_sums_u8(x: torch.Tensor, mode: str = "auto") -> torch.Tensor:
    """sums[j] = sum_r v[r, j] of uint8 samples (include/deig.h deig_colsum_u8): a (d,)
    float64 tensor from an integer accumulation - exact for mode "raw", the integer sum of
    r + g + b divided by 3 (one rounding) for "gray"; deterministic.  x, mode: as
    ``sigma_hat_u8``.  The input of the pooled mean of a centred uint8 fit."""
    x, mode, n, d, dp = _u8_samples(x, mode, "column_sums_u8")
    sums = torch.zeros(dp, dtype=torch.float64, device=x.device)
    if n == 0 or d == 0:
        return sums[:d]
    _call(x.device, "deig_colsum_u8",
          (x.data_ptr(), n, dp, x.stride(0), _lib.U8_MODES[mode], sums.data_ptr()),
          "deig_colsum_u8_workspace", (n, dp))
    return sums[:d].contiguous() if dp != d else sums


def sigma_hat_u8_centered(x: torch.Tensor, center: torch.Tensor | None = None, mode: str = "auto",
                          alpha: float | None = None, dtype: torch.dtype = torch.float64,
                          return_mean: bool = False):
    """Centred covariance alpha * sum_r (v_r - c)(v_r - c)^T of uint8 samples, alpha = 1/n by
    default (include/deig.h deig_syrk_u8_centered): the exact integer pipeline of
    ``sigma_hat_u8`` with centred epilogues - the numerator n sum y_i y_j - Y_i Y_j is formed
    exactly, the result is float64-grade (8 * 2^-53 relative to the terms, see the header).
    x, mode: as ``sigma_hat_u8``.  center: (d,) float64 in units of v (the pooled mean of a
    multi-shard fit), None = this shard's own mean.  Returns a (d, d) tensor of ``dtype``
    (float64 by default; float32 is its rounding), bit-exactly symmetric; with
    ``return_mean`` also the shard's own mean ((d,) float64)."""
    x, mode, n, d, dp = _u8_samples(x, mode, "sigma_hat_u8_centered")
    _check_result_dtype(dtype)
    if n == 0:
        return _nan_cov(d, dtype, x.device, return_mean)
    c = _pad_vector(center, d, dp, x.device, "center")
    S = torch.empty((dp, dp), dtype=dtype, device=x.device)
    mean = torch.empty(dp, dtype=torch.float64, device=x.device) if return_mean else None
    _call(x.device, "deig_syrk_u8_centered",
          (x.data_ptr(), n, dp, x.stride(0), _lib.U8_MODES[mode], _ptr(c), _alpha(alpha, n),
           *_cov_outputs(S, dp, False), _ptr(mean)),
          "deig_syrk_u8_centered_workspace", (n, dp, _lib.U8_MODES[mode]))
    if dp != d:
        S = S[:d, :d].contiguous()
        mean = mean[:d].contiguous() if mean is not None else None
    return (S, mean) if return_mean else S


def pca_transform_u8(X: torch.Tensor, W: torch.Tensor, mean: torch.Tensor | None = None,
                     mode: str = "auto", *, residual: bool = False, energy: bool = False):
    """``pca_transform`` of uint8 samples, the bytes read once (include/deig.h
    deig_pca_transform_u8): Y = (V - mean) W with V the features of X (X, mode: as
    ``sigma_hat_u8``), mean (d,) in units of v or None (no centring), W (d, k) any layout
    with k <= 256.  Centred in double when the bytes are staged, before the product.
    Returns Y, or the tuple (Y[, residual][, energy]) as ``pca_transform``."""
    X, mode, n, d, dp = _u8_samples(X, mode, "pca_transform_u8")
    dev = X.device
    W, mu, k = _transform_operands(W, d, dp, mean, dev, "W")
    W = W.to(dev)
    Y, res, en = _transform_buffers(n, k, dev, residual, energy)
    if n > 0:
        _call(dev, "deig_pca_transform_u8",
              (X.data_ptr(), n, dp, X.stride(0), _lib.U8_MODES[mode], _ptr(mu), W.data_ptr(), k,
               _ld(W, 1, dp), Y.data_ptr(), _ld(Y, 0, k), _ptr(res), _ptr(en)),
              "deig_pca_transform_u8_workspace", (n, dp, k))
    return _transform_result(Y, res, en)


def sigma_hat_u8(x: torch.Tensor, mode: str = "auto", alpha: float | None = None,
                 out: torch.Tensor | None = None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Exact Sigma_hat of uint8 samples on int8 MFMA (fused ingest).

    x: uint8 tensor on the GPU (host arrays are copied over), either
      * (n, d) raw bytes, mode "raw": V = x;
      * (n, H, W, 3) interleaved pixels (CIFAR layout, load_data.py:18-33), mode
        "gray": V = x.mean(axis=3).reshape(n, H*W) - the reference's preprocessing
        distributed.py:170-173 - fused into the covariance; or (n, 3m) rows with
        mode "gray" explicitly.
    Returns alpha * V^T V (alpha = 1/n: distributed.py:59-70) as a (d, d) tensor of
    ``dtype`` (float32: within one ulp of the exact result - a double quotient
    rounded to float; float64: exact to double rounding).  Every product and sum is an integer computation
    (include/deig.h deig_syrk_u8), so there is no accumulation error at all.
    """
    x, mode, n, d, dp = _u8_samples(x, mode, "sigma_hat_u8")
    if n == 0:
        return _nan_cov(d, dtype, x.device)
    _check_result_dtype(dtype)
    direct = (out is not None and dp == d and out.dtype == dtype and out.device == x.device
              and out.shape == (d, d) and out.stride(1) == 1 and out.stride(0) >= d)
    S = out if direct else torch.empty((dp, dp), dtype=dtype, device=x.device)
    _call(x.device, "deig_syrk_u8",
          (x.data_ptr(), n, dp, x.stride(0), _lib.U8_MODES[mode], _alpha(alpha, n),
           *_cov_outputs(S, S.stride(0), False)),
          "deig_syrk_u8_workspace", (n, dp, _lib.U8_MODES[mode]))
    if direct:  # written in place
        return out
    if dp != d:
        S = S[:d, :d].contiguous()
    if out is not None:
        out.copy_(S)
        return out
    return S


# ---------------------------------------------------------------- eigensolvers
def _pad_dim(d: int) -> int:
    return max(16, (d + 3) // 4 * 4)


def _finish(rc, V, evals, sweeps, resid, what):
    """The EigResult of a solve that returned ``rc`` (checked); called by the public op
    itself, so that the warning points at the op's caller."""
    conv = rc == _lib.DEIG_OK
    if not conv:
        warnings.warn(f"{what}: {_lib.last_error()}", _lib.NotConvergedWarning, stacklevel=3)
    return EigResult(evals=evals, V=V, sweeps=int(sweeps.value), resid=float(resid.value),
                     converged=conv)


def _colmajor(d: int, k: int, device) -> torch.Tensor:
    return torch.empty((k, d), dtype=torch.float32, device=device).t()


def _solver_outputs(d: int, k: int, device):
    """(V, evals, sweeps, resid): the device outputs of one solve and its host out-words."""
    return (_colmajor(d, k, device), torch.empty(k, dtype=torch.float32, device=device),
            ctypes.c_int(0), ctypes.c_float(0))


def _warm(q0, d, device):
    if q0 is None:
        return None, 0, d
    q = require_device_tensor(q0, "q0")
    if q.dim() == 1:
        q = q[:, None]
    if q.shape[0] != d:
        raise ValueError(f"q0 must have {d} rows")
    q = q.t().contiguous().t()  # column-major
    return q, q.shape[1], _ld(q, 1, d)


def _solver_matrix(S: torch.Tensor) -> torch.Tensor:
    """S as the solver reads it: unit column stride; when the library reads it in
    place (d % 4 == 0: include/deig.h deig_topk_sym_ex) also a row stride % 4 == 0 and
    16-byte alignment.  Other dimensions are staged by the library itself (a zero-padded
    copy in the workspace whose padding never enters the result), so no padding here."""
    d = S.shape[0]
    if S.stride(1) != 1 or S.stride(0) < d:
        S = S.contiguous()
    if d % 4 == 0 and (S.stride(0) % 4 or S.data_ptr() % 16):
        S = S.clone(memory_format=torch.contiguous_format)
    return S


def topk_eigh(S: torch.Tensor, k: int, *, p: int | None = None, tol: float = DEFAULT_TOL,
              max_sweeps: int = DEFAULT_MAX_SWEEPS, q0: torch.Tensor | None = None,
              check_finite: bool = True, opts: "_lib.SolverOpts | None" = None) -> EigResult:
    """Top-k eigenpairs of a symmetric matrix, ascending (GPU subspace iteration).

    GPU replacement for ``Node.top_k_eigenvectors`` (distributed.py:22-29:
    ``eigh(matrix, eigvals=(N-k, N-1))[1]``) that also returns the eigenvalues.
    Like scipy's ``?syevr`` call it takes any symmetric S of any size d and any
    1 <= k <= d (ValueError outside, like scipy's subset_by_index check): k > 128 runs
    in locked blocks of p - 16 pairs, an indefinite S is detected from the Ritz values
    and solved as S + sigma I, and a d the kernels cannot take as is (d % 4 != 0,
    d < 16, a subspace wider than d) is staged by the library in a padded copy whose
    padding directions never outrank S's own eigenpairs (include/deig.h
    deig_topk_sym_ex).  A float64 S (the reference's dtype) is read in double by the
    image and deflation passes.  Only the lower triangle matters mathematically, but
    the full matrix is read (the SYRK output is bit-exactly symmetric).  ``opts``:
    solver options (``_lib.solver_opts(...)``).
    """
    S = require_device_tensor(S, "topk_eigh", keep_f64=True)
    if S.dim() != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"expected a square matrix, got {tuple(S.shape)}")
    d = S.shape[0]
    k = _check_k(k, d)
    if check_finite and not bool(torch.isfinite(S).all()):
        raise ValueError("array must not contain infs or NaNs")
    S = _solver_matrix(S)
    q, k0, ldq = _warm(q0, d, S.device)
    pp = int(p) if p else 0
    stype = _elem_type(S.dtype)
    o = ctypes.byref(opts if opts is not None else _lib.solver_opts())
    V, evals, sweeps, resid = _solver_outputs(d, k, S.device)
    rc = _call(S.device, "deig_topk_sym_ex",
               (S.data_ptr(), stype, d, S.stride(0), k, pp, int(max_sweeps), tol, _ptr(q), k0, ldq,
                V.data_ptr(), d, evals.data_ptr(), ctypes.byref(sweeps), ctypes.byref(resid), o),
               "deig_topk_workspace_ex", (d, k, pp, stype, o))
    return _finish(rc, V, evals, sweeps, resid, "deig_topk_sym_ex")


def topk_eigh_batch(Ss, k: int, *, p: int | None = None, tol: float = DEFAULT_TOL,
                    max_sweeps: int = DEFAULT_MAX_SWEEPS, check_finite: bool = True,
                    opts: "_lib.SolverOpts | None" = None) -> list:
    """``topk_eigh`` of W same-shape symmetric matrices at once (the logical workers
    of one GPU, each SlaveNode's top_k_eigenvectors of distributed.py:22-29,
    :42-53): the same results as W ``topk_eigh`` calls, the W problems advanced in
    lockstep on the current stream (two interleaved groups on a second, joined
    stream from d = 2048) with each step's sweeps, Grams, small
    Rayleigh-Ritz solves and updates batched across them (include/deig.h
    deig_topk_sym_batch).  Returns a list of EigResult."""
    Ss = [require_device_tensor(S, "topk_eigh_batch", keep_f64=True) for S in Ss]
    if not Ss:
        return []
    S0 = Ss[0]
    if S0.dim() != 2 or S0.shape[0] != S0.shape[1]:
        raise ValueError(f"expected square matrices, got {tuple(S0.shape)}")
    d, dev, dt = S0.shape[0], S0.device, S0.dtype
    for S in Ss:
        if S.shape != S0.shape or S.device != dev or S.dtype != dt:
            raise ValueError("topk_eigh_batch: every matrix must have the same shape, dtype, device")
        if check_finite and not bool(torch.isfinite(S).all()):
            raise ValueError("array must not contain infs or NaNs")
    k = _check_k(k, d)
    mats = [_solver_matrix(S) for S in Ss]
    lds = mats[0].stride(0)
    if any(S.stride(0) != lds for S in mats):
        mats = [S.contiguous() for S in mats]
        lds = d
    W = len(mats)
    pp = int(p) if p else 0
    stype = _elem_type(dt)
    o = ctypes.byref(opts if opts is not None else _lib.solver_opts())
    Vs = [_colmajor(d, k, dev) for _ in range(W)]
    evs = [torch.empty(k, dtype=torch.float32, device=dev) for _ in range(W)]
    sweeps = (ctypes.c_int * W)()
    resid = (ctypes.c_float * W)()
    status = (ctypes.c_int * W)()
    S_arr, V_arr, E_arr = ((ctypes.c_void_p * W)(*[t.data_ptr() for t in ts])
                           for ts in (mats, Vs, evs))
    rc = _call(dev, "deig_topk_sym_batch_ex",
               (W, S_arr, stype, d, lds, k, pp, int(max_sweeps), tol, V_arr, d, E_arr, sweeps,
                resid, status, o),
               "deig_topk_batch_workspace", (W, d, k, pp, stype, o))
    if rc != _lib.DEIG_OK:
        warnings.warn(f"deig_topk_sym_batch_ex: {_lib.last_error()}", _lib.NotConvergedWarning,
                      stacklevel=2)
    # each problem's own outcome (status[i]: what deig_topk_sym_ex would have returned)
    return [EigResult(evals=evs[i], V=Vs[i], sweeps=int(sweeps[i]), resid=float(resid[i]),
                      converged=int(status[i]) == _lib.DEIG_OK) for i in range(W)]


def stack_bases(bases) -> torch.Tensor:
    """[V_1, ..., V_m] (each d x k) -> Wt = [V_1^T; ...; V_m^T]  ((m k) x d row-major)."""
    rows = [require_device_tensor(v, "basis").t() for v in bases]
    return torch.cat(rows, dim=0).contiguous()


def projavg_topk(Wt: torch.Tensor, k: int, scale: float, *, p: int | None = None,
                 tol: float = DEFAULT_TOL, max_sweeps: int = DEFAULT_MAX_SWEEPS,
                 q0: torch.Tensor | None = None,
                 opts: "_lib.SolverOpts | None" = None) -> EigResult:
    """Top-k eigenpairs of scale * sum_i V_i V_i^T, never forming the d x d matrix.

    GPU replacement for MasterNode.callback_ (distributed.py:126-130:
    sigma_tilde = sum V V^T / batches_number) followed by the notebook's server
    solve (Online Distributed PCA.ipynb raw line 306).  Wt = stack_bases(...)
    is (m k) x d row-major; rows may carry per-basis weights (online variant).
    """
    Wt = require_device_tensor(Wt, "projavg_topk")
    if Wt.dim() != 2:
        raise ValueError("Wt must be 2-D ((m k) x d)")
    mk, d = Wt.shape
    k = _check_k(k, d)
    dp = _pad_dim(d)
    if not p:
        dp = max(dp, default_subspace(max(dp, (min(k, MAX_P) + 15) // 16 * 16), k))
    Wt = _stack_4(Wt, dp)
    q, k0, ldq = _warm(q0, d, Wt.device)
    if q is not None and dp != d:
        qp = torch.zeros((dp, k0), dtype=torch.float32, device=Wt.device)
        qp[:d] = q
        q, ldq = qp.t().contiguous().t(), dp
    pp = int(p) if p else default_subspace(dp, k)
    o = ctypes.byref(opts if opts is not None else _lib.solver_opts())
    V, evals, sweeps, resid = _solver_outputs(dp, k, Wt.device)
    rc = _call(Wt.device, "deig_projavg_topk_ex",
               (Wt.data_ptr(), dp, mk, Wt.stride(0), scale, k, pp, int(max_sweeps), tol, _ptr(q),
                k0, ldq, V.data_ptr(), dp, evals.data_ptr(), ctypes.byref(sweeps),
                ctypes.byref(resid), o),
               "deig_projavg_workspace_ex", (dp, mk, k, pp, o))
    res = _finish(rc, V, evals, sweeps, resid, "deig_projavg_topk_ex")
    if dp != d:
        res.V = res.V[:d].t().contiguous().t()
    return res


# ---------------------------------------------------------------- covariance-free route
def _sample_operands(X, center, name: str):
    """``(X, xtype, n, d, dp, center)`` of a covariance-free call: the samples as
    ``_packed_samples`` gives them with d >= 16, ``center`` as ``_pad_vector`` does.  float64
    samples raise: the route's products are float32."""
    if str(getattr(X, "dtype", "")).endswith("float64"):
        raise TypeError(f"{name}: float64 samples are not supported by the covariance-free route; "
                        "use the explicit route (sigma_hat / sigma_hat_centered + topk_eigh), which "
                        "reads float64 in double")
    X, xtype, n, d, dp = _packed_samples(X, name, "X", 16)
    if n < 1:
        raise ValueError(f"{name}: X must be 2-D with at least one row, got shape {tuple(X.shape)}")
    return X, xtype, n, d, dp, _pad_vector(center, d, dp, X.device, "center")


def gram_apply(X: torch.Tensor, Q: torch.Tensor, center=None, alpha: float | None = None) -> torch.Tensor:
    """``alpha * Xc^T (Xc Q)`` for the n x d samples X (float32, bfloat16 or uint8 raw bytes)
    about ``center`` (d values, taken in float64; None: no centring), without forming d x d:
    the operator of ``topk_samples`` (include/deig.h deig_gram_apply).  Q: (d, p) with p a
    multiple of 16 in 16..128; alpha defaults to 1/n.  Returns the (d, p) float32 product."""
    X, xtype, n, d, dp, c = _sample_operands(X, center, "gram_apply")
    Q = require_device_tensor(Q, "Q")
    if Q.dim() != 2 or Q.shape[0] != d or Q.device != X.device:
        raise ValueError(f"Q must be a (d, p) = ({d}, p) tensor on X's device, got {tuple(Q.shape)}")
    p = Q.shape[1]
    if dp != d:
        Qp = torch.zeros((dp, p), dtype=torch.float32, device=X.device)
        Qp[:d] = Q
        Q = Qp
    elif Q.stride(1) != 1 or Q.stride(0) % 4 or Q.stride(0) < p or Q.data_ptr() % 16:
        Q = Q.clone(memory_format=torch.contiguous_format)
    Y = torch.empty((dp, p), dtype=torch.float32, device=X.device)
    _call(X.device, "deig_gram_apply",
          (X.data_ptr(), xtype, n, dp, _ld(X, 0, dp), _ptr(c), _alpha(alpha, n), Q.data_ptr(), p,
           _ld(Q, 0, p), Y.data_ptr(), p),
          "deig_gram_apply_workspace", (n, dp, p, xtype))
    return Y[:d] if dp != d else Y


def topk_samples(X: torch.Tensor, k: int, center=None, alpha: float | None = None, *,
                 p: int | None = None, tol: float = DEFAULT_TOL, max_sweeps: int = DEFAULT_MAX_SWEEPS,
                 q0: torch.Tensor | None = None, opts: "_lib.SolverOpts | None" = None) -> EigResult:
    """Top-k eigenpairs (ascending) of ``alpha * Xc^T Xc`` straight from the n x d samples,
    never forming the d x d covariance: the covariance-free worker route (include/deig.h
    deig_topk_samples).  X: float32, bfloat16 or uint8 (raw bytes) samples, read where they
    lie; ``center``: d values subtracted in double where a sample is staged (None: none);
    alpha defaults to 1/n; 1 <= k <= 128.  Two reads of X per solver sweep, workspace
    O((n_chunk + d) p): the route for n << d and for d beyond the covariance kernels.  The
    operator is implicit, so a dominant mean direction is not deflated: centre such data
    (``center=``) or use ``sigma_hat*`` + ``topk_eigh``."""
    X, xtype, n, d, dp, c = _sample_operands(X, center, "topk_samples")
    k = _check_k(k, d)
    q, k0, ldq = _warm(q0, d, X.device)
    if q is not None and dp != d:
        qp = torch.zeros((dp, k0), dtype=torch.float32, device=X.device)
        qp[:d] = q
        q, ldq = qp.t().contiguous().t(), dp
    pp = int(p) if p else default_subspace(dp, k)
    o = ctypes.byref(opts if opts is not None else _lib.solver_opts())
    V, evals, sweeps, resid = _solver_outputs(dp, k, X.device)
    rc = _call(X.device, "deig_topk_samples",
               (X.data_ptr(), xtype, n, dp, _ld(X, 0, dp), _ptr(c), _alpha(alpha, n), k, pp,
                int(max_sweeps), tol, _ptr(q), k0, ldq, V.data_ptr(), dp, evals.data_ptr(),
                ctypes.byref(sweeps), ctypes.byref(resid), o),
               "deig_topk_samples_workspace", (n, dp, k, pp, xtype, o))
    res = _finish(rc, V, evals, sweeps, resid, "deig_topk_samples")
    if dp != d:
        res.V = res.V[:d].t().contiguous().t()
    return res


# ---------------------------------------------------------------- wide-data (dual) route
def gram_outer(X: torch.Tensor, center=None, alpha: float | None = None) -> torch.Tensor:
    """``alpha * Xc Xc^T``, the (n, n) float32 sample-space Gram matrix of the n x d samples X
    (float32, bfloat16 or uint8 raw bytes) about ``center`` (d values, taken in float64; None:
    no centring) on the bf16 MFMA (include/deig.h deig_gram_outer): bit-exactly symmetric,
    n <= 32768; alpha defaults to 1/n.  The matrix of ``topk_dual``."""
    X, xtype, n, d, dp, c = _sample_operands(X, center, "gram_outer")
    ldk = -(-n // 4) * 4
    K = torch.empty((n, ldk), dtype=torch.float32, device=X.device)
    _call(X.device, "deig_gram_outer",
          (X.data_ptr(), xtype, n, dp, _ld(X, 0, dp), _ptr(c), _alpha(alpha, n), K.data_ptr(), ldk, 0),
          "deig_gram_outer_workspace", (n, dp, xtype, int(c is not None)))
    return K[:, :n] if ldk != n else K


def topk_dual(X: torch.Tensor, k: int, center=None, alpha: float | None = None, *,
              p: int | None = None, tol: float = DEFAULT_TOL, max_sweeps: int = DEFAULT_MAX_SWEEPS,
              opts: "_lib.SolverOpts | None" = None) -> EigResult:
    """Top-k eigenpairs (ascending) of ``alpha * Xc^T Xc`` through the n x n Gram matrix of the
    samples: the wide-data worker route (include/deig.h deig_topk_dual) for n <= d, n <= 32768.
    ``gram_outer`` on the bf16 MFMA, its top-k by the explicit solver, one back-projection, and
    a finish by ``topk_samples``'s solver from that start - so the result, its stopping rule
    and ``sweeps`` (the finish's) are ``topk_samples``'s, and so is its caveat: a dominant mean
    direction is not deflated, centre such data.  Arguments as for ``topk_samples``;
    1 <= k <= min(128, n, d)."""
    if len(getattr(X, "shape", ())) == 2 and int(k) > X.shape[0]:  # before X moves anywhere
        raise ValueError(f"topk_dual: k={int(k)} exceeds the n={X.shape[0]} rows of X (the Gram "
                         "matrix is n x n)")
    X, xtype, n, d, dp, c = _sample_operands(X, center, "topk_dual")
    k = _check_k(k, d)
    pp = int(p) if p else default_subspace(dp, k)
    o = ctypes.byref(opts if opts is not None else _lib.solver_opts())
    V, evals, sweeps, resid = _solver_outputs(dp, k, X.device)
    rc = _call(X.device, "deig_topk_dual",
               (X.data_ptr(), xtype, n, dp, _ld(X, 0, dp), _ptr(c), _alpha(alpha, n), k, pp,
                int(max_sweeps), tol, V.data_ptr(), dp, evals.data_ptr(), ctypes.byref(sweeps),
                ctypes.byref(resid), o),
               "deig_topk_dual_workspace", (n, dp, k, pp, xtype, o))
    res = _finish(rc, V, evals, sweeps, resid, "deig_topk_dual")
    if dp != d:
        res.V = res.V[:d].t().contiguous().t()
    return res


# ---------------------------------------------------------------- Procrustes average
@dataclass
class ProcrustesResult:
    """Procrustes-aligned average of a stack of bases (``procrustes_average``)."""

    V: torch.Tensor        # (d, k) float32, column-major; columns follow the reference basis
    cosines: torch.Tensor  # (m, k) cosines of the principal angles basis i / reference, descending
    Z: torch.Tensor        # (m, k, k) the alignment rotations Z_i (last pass)


def _colmajor_basis(t, d: int, k: int, dp: int, device, name: str) -> torch.Tensor:
    """(d, k) basis as a column-major float32 tensor of dp >= d rows (zero padded)."""
    t = require_device_tensor(t, name)
    if t.dim() != 2 or tuple(t.shape) != (d, k):
        raise ValueError(f"{name} must have shape ({d}, {k}), got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} must live on {device}")
    out = torch.zeros((k, dp), dtype=torch.float32, device=device)
    out[:, :d] = t.t()
    return out.t()


def procrustes_average(Wt: torch.Tensor, k: int, *, ref=None, weights=None,
                       iters: int = 1) -> ProcrustesResult:
    """V = orth(sum_i w_i V_i Z_i) with Z_i the orthogonal Procrustes rotation of V_i onto
    the reference basis (include/deig.h deig_procrustes_avg_f32): the one-pass
    aggregator of Charisopoulos, Benson and Damle.  No eigensolve, and the columns of V
    follow the reference's columns (``projavg_topk`` fixes only the span).

    Wt = stack_bases(...) is (m k) x d row-major.  ref: None (the first basis of the
    stack), an integer index into the stack, or a (d, k) tensor.  weights: m non-negative
    numbers, not all zero (None: equal).  iters (1..8): pass t > 1 aligns to the result
    of pass t - 1.  k <= 128.
    """
    Wt = require_device_tensor(Wt, "procrustes_average")
    if Wt.dim() != 2:
        raise ValueError("Wt must be 2-D ((m k) x d)")
    mk, d = Wt.shape
    k = _check_k(k, d)
    if k > MAX_P:
        raise ValueError(f"procrustes_average takes k <= {MAX_P}; use projavg_topk above")
    if mk < k or mk % k:
        raise ValueError(f"Wt has {mk} rows, not a positive multiple of k={k}")
    m = mk // k
    dev = Wt.device
    dp = _pad_dim(d)
    Wt = _stack_4(Wt, dp)
    rptr, ldref, rkeep = None, dp, None
    if ref is not None:
        if isinstance(ref, int):
            if not 0 <= ref < m:
                raise ValueError(f"ref index {ref} out of range [0, {m})")
            # basis i of the stack: its k rows are the column-major d x k bytes
            rkeep = Wt[ref * k:(ref + 1) * k]
            ldref = Wt.stride(0)
        else:
            rkeep = _colmajor_basis(ref, d, k, dp, dev, "ref")
            ldref = rkeep.stride(1)
        rptr = rkeep.data_ptr()
    wptr = None
    if weights is not None:
        wl = [float(x) for x in (weights.tolist() if hasattr(weights, "tolist") else weights)]
        if len(wl) != m:
            raise ValueError(f"weights must hold m = {m} numbers, got {len(wl)}")
        wptr = (ctypes.c_float * m)(*wl)
    V = _colmajor(dp, k, dev)
    Z = torch.empty((m, k, k), dtype=torch.float32, device=dev)
    cos = torch.empty((m, k), dtype=torch.float32, device=dev)
    _call(dev, "deig_procrustes_avg_f32",
          (Wt.data_ptr(), dp, mk, Wt.stride(0), k, rptr, ldref, wptr, int(iters), V.data_ptr(), dp,
           Z.data_ptr(), cos.data_ptr()),
          "deig_procrustes_workspace", (dp, mk, k))
    if dp != d:
        V = V[:d].t().contiguous().t()
    return ProcrustesResult(V=V, cosines=cos, Z=Z)


def subspace_distance(A: torch.Tensor, B: torch.Tensor):
    """(||sin Theta(A, B)||_F, ||sin Theta(A, B)||_2) of the spans of two orthonormal
    (d, k) bases, computed on the device from the residual B - A (A^T B)
    (include/deig.h deig_subspace_dist_f32): unlike the cosine forms it resolves
    distances far below 1e-3 in float32.  Synchronises to return Python floats."""
    A = require_device_tensor(A, "subspace_distance")
    if A.dim() != 2:
        raise ValueError("A must be a (d, k) basis")
    d, k = A.shape
    if not 1 <= k <= min(d, MAX_P):
        raise ValueError(f"k={k} out of range [1, min(d, {MAX_P})]")
    dev = A.device
    dp = _pad_dim(d)
    Ac = _colmajor_basis(A, d, k, dp, dev, "A")
    Bc = _colmajor_basis(B, d, k, dp, dev, "B")
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _call(dev, "deig_subspace_dist_f32",
          (Ac.data_ptr(), Ac.stride(1), Bc.data_ptr(), Bc.stride(1), dp, k, out.data_ptr()),
          "deig_subspace_dist_workspace", (dp, k))
    fro, two = out.tolist()
    return fro, two


def projector_distance(A: torch.Tensor, B: torch.Tensor) -> float:
    """||A A^T - B B^T||_F = sqrt(2) ||sin Theta(A, B)||_F of two orthonormal (d, k)
    bases (``subspace_distance``)."""
    return 2.0 ** 0.5 * subspace_distance(A, B)[0]


# ---------------------------------------------------------------- Oja
def oja_step(Xb: torch.Tensor, V: torch.Tensor, eta: float, center=None) -> torch.Tensor:
    """In-place mini-batch Oja update V <- orth(V + eta/b Xb^T Xb V) (config 4).

    Not in the reference (parity unpinned).  V: (d, k) column-major float32
    (as returned by topk_eigh), k <= 64.  Returns V.  A bfloat16 Xb is consumed as
    bfloat16 under the rules of ``oja_steps`` (no float32 copy, and the call stays
    asynchronous: that route cannot time out); so is a uint8 Xb, and ``center`` (a (d,)
    float64 tensor: the step is taken on ``Xb - center``) works as it does there.
    """
    if center is not None:
        return _oja_steps_centered(Xb, V, eta, None, 1, center, "oja_step", "Xb")
    xb = _oja_reads_in_place(Xb, V, "auto", Xb.shape[0] if isinstance(Xb, torch.Tensor) else 0, "oja_step")
    if xb is not None:
        return _oja_steps_centered(xb, V, eta, None, 1, None, "oja_step", "Xb")
    Xb = _rowmajor(require_device_tensor(Xb, "oja_step"), "Xb")
    b, d = Xb.shape
    k = _oja_basis(V, Xb, "Xb")
    _call(Xb.device, "deig_oja_step_f32",
          (Xb.data_ptr(), b, d, Xb.stride(0), eta, V.data_ptr(), k, _ld(V, 1, d)),
          "deig_oja_workspace", (b, d, k))
    oja_check(Xb.device, b, d, k)
    return V


def _oja_basis(V: torch.Tensor, X: torch.Tensor, xname: str) -> int:
    """Check Oja's basis against the samples X (named ``xname``): (d, k) column-major
    float32 on X's device.  Returns k."""
    if V.dim() != 2 or V.shape[0] != X.shape[1] or V.stride(0) != 1 or V.dtype != torch.float32 \
            or V.device != X.device:
        raise ValueError(f"V must be a (d, k) column-major float32 tensor on {xname}'s device")
    return V.shape[1]


def _oja_reads_in_place(X, V, algo: str, batch: int, name: str) -> torch.Tensor | None:
    """The bfloat16 or uint8 samples of an uncentred Oja call, on the device, where the
    two-pass route (deig_oja_steps_centered with a NULL centre) can read them in place; None
    when the call keeps the float32 route: another dtype, ``algo="resident"``, a view the
    entry point cannot read in place (``_in_place``), or - uint8 only - ``algo="auto"`` at the
    resident-eligible shape (whose bits are the resident kernel's, not the two-pass
    kernels')."""
    if not isinstance(X, torch.Tensor) or X.dtype not in (torch.bfloat16, torch.uint8) \
            or algo not in ("auto", "two_pass") or X.dim() != 2 or X.shape[0] < 1:
        return None
    if X.dtype == torch.uint8:
        if not isinstance(V, torch.Tensor) or V.dim() != 2:
            return None
        d = X.shape[1]
        if algo == "auto" and batch == 4096 and d % 512 == 0 and 0 < d <= 3072 and V.shape[1] <= 32:
            return None
    X = _to_device(X, name)
    return X if _in_place(X) else None


def _oja_steps_centered(X, V: torch.Tensor, eta: float, batch, orth_every: int, center, name: str,
                        xname: str) -> torch.Tensor:
    """Batches of ``batch`` rows (None: all of X is one batch) through
    deig_oja_steps_centered on the samples as ``_packed_samples`` gives them, with ``center``
    and V zero-padded to a padded copy's columns (its row of V stays zero).  No
    ``oja_check``: the route cannot time out, and the call stays asynchronous."""
    X, xtype, n, d, dp = _packed_samples(X, name, xname)
    b = n if batch is None else int(batch)
    nb = n // b if b > 0 else 0
    if nb < 1:
        raise ValueError(f"need at least one full batch of {batch} rows, got {n} rows")
    c = _pad_vector(center, d, dp, X.device, "center")
    Vc = V
    if dp != d and isinstance(V, torch.Tensor) and V.dim() == 2 and V.shape[0] == d:
        Vc = torch.zeros((V.shape[1], dp), dtype=V.dtype, device=V.device).t()
        Vc[:d] = V
    k = _oja_basis(Vc, X, xname)
    _call(X.device, "deig_oja_steps_centered",
          (X.data_ptr(), xtype, nb, b, dp, _ld(X, 0, dp), _ptr(c), eta, Vc.data_ptr(), k,
           _ld(Vc, 1, dp), int(orth_every)),
          "deig_oja_workspace", (b, dp, k))
    if Vc is not V:
        V.copy_(Vc[:d])
    return V


def oja_check(device, b: int, d: int, k: int) -> None:
    """Raise ``DeigTimeoutError`` if the last Oja call on this thread's workspace for
    (b, d, k) on ``device`` timed out in a resident hand-off (its basis is NaN);
    synchronises that device's current stream (include/deig.h deig_oja_error)."""
    L = _lib.lib()
    with torch.cuda.device(device):
        nbytes = L.deig_oja_workspace(b, d, k)
        ws = _workspace(device, nbytes)
        rc = L.deig_oja_error(ws.data_ptr(), nbytes, b, d, k, _stream(device))
    _lib.check(rc, "oja")


def oja_steps(X: torch.Tensor, V: torch.Tensor, eta: float, batch: int,
              orth_every: int = 8, algo: str = "auto", check: bool = True, center=None) -> torch.Tensor:
    """In-place Oja over the consecutive row batches X[i*batch:(i+1)*batch] (config 4).

    One C call for all batches (no host work in between); the basis is
    re-orthonormalised every ``orth_every`` batches and at the end, which gives the
    span of per-batch orthonormalisation (``oja_step`` in a loop) because the update
    is linear in V.  Rows beyond the last full batch are ignored.  ``algo``
    (include/deig.h DEIG_OJA_*): "auto", "two_pass" or "resident" (Xb read once per
    batch; batch = 4096, d a multiple of 512 up to 3072, k <= 32).  ``check`` (default):
    synchronise and raise ``DeigTimeoutError`` if a resident hand-off timed out (V is
    then NaN); ``check=False`` leaves the call asynchronous - then call ``oja_check``
    before any other op on this thread's stream (they share the workspace that holds
    the timeout word).  Returns V.

    bfloat16 samples are consumed as bfloat16 (include/deig.h deig_oja_steps_centered without
    a centre, which is deig_oja_steps_bf16 bit for bit: the
    two-pass kernels with the sample as the MFMA operand, two products per fragment pair
    instead of three, no float32 copy; the bits of ``algo="two_pass"`` on ``X.float()``)
    when ``algo`` is "auto" or "two_pass" and X is a 2-D view with unit column stride,
    d % 8 == 0, a row stride % 8 == 0 and a 16-byte aligned base - a row-strided view
    such as ``x[:, :d]`` is read in place.  That route cannot time out: it makes no
    ``oja_check`` call and stays asynchronous whatever ``check`` says.  Any other
    bfloat16 input (``algo="resident"``, d % 8 == 4, odd strides) is widened to float32
    first, as every bfloat16 input was before.  "auto" takes the bfloat16 kernels at every
    shape, resident-eligible ones included: at config 4's shape (batch 4096, d = 3072,
    k = 32, 64 batches, orth_every 8) they took 31.6 us per batch against 40.1 us for
    widening plus the resident kernel and 50.0 us for widening plus the float32 two-pass
    kernels, and at 4096 x 8192, k = 64, 84.8 against 140.1 us (profiles/oja_bf16.json,
    tools/oja_bf16_bench.py).

    ``center``: a (d,) float64 tensor (other dtypes and devices are converted), for
    example ``PCA.mean_``: the steps are taken on ``X - center``.  Every dtype then goes
    through include/deig.h deig_oja_steps_centered: each sample is centred where the
    kernels stage it, ``fl32(float64(x) - center)`` with one rounding, and the result has
    the bits of ``algo="two_pass"`` on the float32 tensor ``(X.double() - center).float()``
    without that tensor.  uint8, bfloat16 and float32 samples (anything else becomes
    float32) are read in place under their layout rules - unit column stride, d and the row
    stride % 4 == 0 (bfloat16: % 8), a 16-byte (uint8: 4-byte) aligned base; any other view
    is copied into a zero-padded tensor of the same dtype, never a float32 one.  There is no
    resident centred kernel: ``algo="resident"`` with a centre is a ValueError, and the
    call makes no ``oja_check`` and stays asynchronous whatever ``check`` says.

    uint8 samples without a centre are read in place as bytes too (a byte is exact in
    bfloat16: two products per fragment pair, the bits of ``algo="two_pass"`` on
    ``X.float()``) for "two_pass", and for "auto" except at the resident-eligible shape
    (batch 4096, d % 512 == 0, d <= 3072, k <= 32), where the samples are widened and the
    library chooses, as before: no existing call changes its bits.

    Measured per batch, CholQR included (profiles/oja_centered.json,
    tools/oja_centered_bench.py): the centred call in place took 39.3 /
    34.8 / 34.4 us (float32 / bfloat16 / uint8) at config 4's shape against 144 to 146 us
    for materialising ``(X.double() - center).float()`` and running float32 two-pass, and
    132.6 / 94.8 / 95.4 against 388 to 396 us at 4096 x 8192, k = 64 - the in-place float32
    call is faster than materialising too.  Centring costs 10 to 13 % over the uncentred
    bfloat16 / uint8 kernels (34.8 against 31.6 us, 34.4 against 30.5 us): the third
    product, the double subtraction and the mean loads together, which the run does not
    separate.  uint8 bytes in place without a centre: 30.5 us against 59.0 us for widening
    plus "auto" at config 4's shape, 84.9 against 185.8 us at 4096 x 8192."""
    b = int(batch)
    if center is not None:
        if algo not in _lib.OJA_ALGOS:
            raise ValueError(f"algo must be one of {sorted(_lib.OJA_ALGOS)}, got {algo!r}")
        if algo == "resident":
            raise ValueError("oja_steps: there is no centred resident kernel; use algo='auto' or "
                             "'two_pass' with a center")
        return _oja_steps_centered(X, V, eta, b, orth_every, center, "oja_steps", "X")
    xp = _oja_reads_in_place(X, V, algo, b, "oja_steps")
    if xp is not None and 0 < b <= xp.shape[0]:
        return _oja_steps_centered(xp, V, eta, b, orth_every, None, "oja_steps", "X")
    X = _rowmajor(require_device_tensor(X, "oja_steps"), "X")
    n, d = X.shape
    nb = n // b if b > 0 else 0
    if nb < 1:
        raise ValueError(f"need at least one full batch of {batch} rows, got {n} rows")
    k = _oja_basis(V, X, "X")
    _call(X.device, "deig_oja_steps_ex",
          (X.data_ptr(), nb, b, d, X.stride(0), eta, V.data_ptr(), k, _ld(V, 1, d), int(orth_every),
           _lib.OJA_ALGOS[algo]),
          "deig_oja_workspace", (b, d, k))
    if check:
        oja_check(X.device, b, d, k)
    return V


# ---------------------------------------------------------------- sweep
def sym_apply(S: torch.Tensor, Q: torch.Tensor, algo: str = "auto", alpha: float = 1.0,
              out: torch.Tensor | None = None, prepared: bool = False,
              round_q: bool = False, fast: bool = False, half: bool = False,
              kernel_only: bool = False) -> torch.Tensor:
    """Y = alpha * S Q for symmetric S (d x d) and Q (d x p, p % 16 == 0, p <= 128):
    one subspace-iteration sweep of ``topk_eigh`` (include/deig.h DEIG_SWEEP_*):
    algo "bf16x6" (default via "auto") or "fp32".  ``prepared=True`` (bf16x6) reuses
    the sweep image of S left in this stream's workspace by the previous call with
    the same S and p (DEIG_SWEEP_PREPARED), as the solver does between sweeps.
    ``round_q=True`` (bf16x6, the solver's mode, DEIG_SWEEP_ROUND_Q): Q (contiguous,
    modified in place) is rounded to its two leading bf16 pieces and Y = alpha S Q'
    is formed from five bf16 products.  ``fast=True`` (implies round_q; the solver's
    early-sweep mode, DEIG_SWEEP_FAST): S is also taken as its two leading bf16
    pieces, three products, ~2^-16 relative.  ``half=True`` (implies fast; the
    solver's first sweeps, DEIG_SWEEP_HALF, p >= 64): S and Q as their leading bf16
    piece alone, one product, ~2^-9 relative.  ``kernel_only=True`` (measurement,
    DEIG_SWEEP_KERNEL_ONLY): only the sweep kernel runs, on the Q image the previous
    call in this stream's workspace left; ``out`` is not written."""
    fast = fast or half
    round_q = round_q or fast
    if algo not in _lib.SWEEP_ALGOS:
        raise ValueError(f"algo must be one of {sorted(_lib.SWEEP_ALGOS)}, got {algo!r}")
    S, Q, d, p = _sweep_operands(S, Q, "sym_apply")
    if round_q:
        if algo == "fp32" or not Q.is_contiguous() or Q.dtype != torch.float32:
            raise ValueError("round_q needs algo bf16x6/auto and a contiguous float32 Q "
                             "(it is rounded in place)")
    Q = Q.contiguous()
    Y = out if out is not None else torch.empty((d, p), dtype=torch.float32, device=S.device)
    code = _sweep_code(_lib.SWEEP_ALGOS[algo], prepared, round_q, fast, half)
    if kernel_only:
        if code & 0xff == _lib.DEIG_SWEEP_FP32:
            raise ValueError("kernel_only needs algo bf16x6/auto")
        code |= _lib.DEIG_SWEEP_KERNEL_ONLY | _lib.DEIG_SWEEP_PREPARED
    _call(S.device, "deig_sym_apply_f32",
          (S.data_ptr(), d, S.stride(0), Q.data_ptr(), p, Q.stride(0), Y.data_ptr(), Y.stride(0),
           alpha, code),
          "deig_sym_apply_workspace", (d, p, code))
    return Y


def _sweep_operands(S, Q, name: str):
    """``(S, Q, d, p)``: the operands of a sweep on the device, S checked as the kernels
    read it (square, row-major, d % 4 == 0, aligned) and Q as d x p."""
    S = require_device_tensor(S, name)
    Q = require_device_tensor(Q, "Q")
    d = S.shape[0]
    if S.dim() != 2 or S.shape[1] != d or Q.dim() != 2 or Q.shape[0] != d:
        raise ValueError(f"shape mismatch: S {tuple(S.shape)}, Q {tuple(Q.shape)}")
    if d % 4 or S.stride(1) != 1 or S.stride(0) % 4 or S.data_ptr() % 16:
        raise ValueError("S must be row-major with d % 4 == 0 and a 16-byte aligned, %4 stride")
    return S, Q, d, Q.shape[1]


def _sweep_code(code: int, prepared: bool, round_q: bool, fast: bool, half: bool) -> int:
    """The algorithm ``code`` with the DEIG_SWEEP_* flag bits of a sweep's mode."""
    if prepared and code != _lib.DEIG_SWEEP_FP32:
        code |= _lib.DEIG_SWEEP_PREPARED
    if round_q:
        code |= _lib.DEIG_SWEEP_ROUND_Q
    if fast:
        code |= _lib.DEIG_SWEEP_FAST
    if half:
        code |= _lib.DEIG_SWEEP_HALF
    return code


def sym_power(S: torch.Tensor, Q: torch.Tensor, cs: torch.Tensor, steps: int,
              out: torch.Tensor | None = None, prepared: bool = False,
              round_q: bool = False, fast: bool = False, half: bool = False) -> torch.Tensor:
    """``steps`` sweeps of the solver's power chain (include/deig.h
    deig_sym_power_f32): Y = S Q, then Q_j <- cs_j Y_j on the columns with
    cs_j > 0, each step fused into the sweep's split-K reduction with the next
    sweep's Q image, as between the Rayleigh-Ritz steps of ``topk_eigh``.  Q
    (contiguous float32, d x p) is updated in place; returns Y = S Q_{steps-1}.
    Flags as for ``sym_apply`` (bf16x6 only)."""
    fast = fast or half
    round_q = round_q or fast
    S, Q, d, p = _sweep_operands(S, Q, "sym_power")
    if not Q.is_contiguous() or Q.dtype != torch.float32:
        raise ValueError("Q must be a contiguous float32 tensor (updated in place)")
    cs = cs.to(device=S.device, dtype=torch.float32).contiguous()
    if cs.numel() != p:
        raise ValueError(f"cs must hold p = {p} column scales")
    Y = out if out is not None else torch.empty((d, p), dtype=torch.float32, device=S.device)
    code = _sweep_code(_lib.DEIG_SWEEP_BF16X6, prepared, round_q, fast, half)
    _call(S.device, "deig_sym_power_f32",
          (S.data_ptr(), d, S.stride(0), Q.data_ptr(), p, Q.stride(0), Y.data_ptr(), Y.stride(0),
           cs.data_ptr(), int(steps), code),
          "deig_sym_apply_workspace", (d, p, code))
    return Y


# ---------------------------------------------------------------- projection
def project(X: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """Y = X W  (NB:345 ``X @ matrix_w``): X (n, d) row-major, W (d, k) any layout."""
    X = _rowmajor(require_device_tensor(X, "project"), "X")
    n, dp = X.shape
    dev = X.device
    W, _, k = _transform_operands(W, None, dp, None, dev, "matrix_w")
    Y, _, _ = _transform_buffers(n, k, dev, False, False)
    _call(dev, "deig_project_f32",
          (X.data_ptr(), n, dp, _ld(X, 0, dp), W.data_ptr(), k, _ld(W, 1, dp), Y.data_ptr(),
           _ld(Y, 0, k)),
          "deig_project_workspace", (n, dp, k))
    return Y


def pca_transform(X: torch.Tensor, W: torch.Tensor, mean: torch.Tensor | None = None, *,
                  residual: bool = False, energy: bool = False):
    """Y = (X - mean) W in one pass over X (include/deig.h deig_pca_transform_f32), and from
    the same pass, on request, ``energy`` (||x_i - mean||^2 per row) and ``residual``
    (max(0, energy_i - ||y_i||^2): for an orthonormal W the squared reconstruction error,
    accurate to a multiple of eps * energy_i, not of eps * residual_i).

    X (n, d) row-major, W (d, k) any layout with k <= 256, mean (d,) or None (no
    centring).  The mean is subtracted in double before the product.  float64 X is centred
    in float64 here and then rounded to float32 (the kernel reads float32); bfloat16 X is
    read as it is (deig_pca_transform_bf16: widened and centred when staged).  Returns Y, or
    the tuple (Y[, residual][, energy])."""
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(X)
    bf16 = X.dtype == torch.bfloat16
    mu = None
    if mean is not None:
        mu = torch.as_tensor(mean).to(dtype=torch.float64).reshape(-1)
    if X.dtype == torch.float64 and mu is not None:
        X = require_device_tensor(X, "pca_transform", keep_f64=True)
        X, mu = (X - mu.to(X.device)).to(torch.float32), None
    q = 8 if bf16 else 4
    X = _rowmajor(_to_device(X, "pca_transform") if bf16 else require_device_tensor(X, "pca_transform"), "X", q)
    n, dp = X.shape
    dev = X.device
    W, mu, k = _transform_operands(W, None, dp, mu, dev, "W", q)
    Y, res, en = _transform_buffers(n, k, dev, residual, energy)
    if n > 0:
        _call(dev, "deig_pca_transform_bf16" if bf16 else "deig_pca_transform_f32",
              (X.data_ptr(), n, dp, _ld(X, 0, dp), _ptr(mu), W.data_ptr(), k, _ld(W, 1, dp),
               Y.data_ptr(), _ld(Y, 0, k), _ptr(res), _ptr(en)),
              "deig_pca_transform_bf16_workspace" if bf16 else "deig_pca_transform_workspace", (n, dp, k))
    return _transform_result(Y, res, en)


# ---------------------------------------------------------------- building block
def gemm_skinny(A: torch.Tensor, B: torch.Tensor, trans_a: bool, alpha: float = 1.0,
                beta: float = 0.0, C: torch.Tensor | None = None) -> torch.Tensor:
    """C = alpha * op(A) @ B + beta * C on the solvers' skinny fp32-MFMA kernel.

    trans_a: A is (K, M) and op(A) = A^T; else A is (M, K).  B is (K, N) with
    N % 16 == 0 and N <= 256.  All row-major float32 on one device: A and B with
    another column stride are copied; C (written in place, returned) must be an
    (M, N) float32 tensor on A's device with unit column stride."""
    A = require_device_tensor(A, "A")
    B = require_device_tensor(B, "B")
    if A.dim() != 2 or B.dim() != 2:
        raise ValueError(f"A and B must be 2-D, got {tuple(A.shape)} and {tuple(B.shape)}")
    if B.device != A.device:
        raise ValueError("A and B must live on one device")
    K, M = (A.shape if trans_a else (A.shape[1], A.shape[0]))
    N = B.shape[1]
    if B.shape[0] != K:
        raise ValueError("inner dimensions differ")
    if A.stride(1) != 1:
        A = A.contiguous()
    if B.stride(1) != 1:
        B = B.contiguous()
    if C is None:
        C = torch.zeros((M, N), dtype=torch.float32, device=A.device)
    elif not isinstance(C, torch.Tensor) or C.dim() != 2 or tuple(C.shape) != (M, N) \
            or C.dtype != torch.float32 or C.device != A.device or C.stride(1) != 1:
        raise ValueError(f"C must be a ({M}, {N}) float32 tensor on A's device with unit "
                         "column stride")
    _call(A.device, "deig_gemm_skinny_f32",
          (int(trans_a), A.data_ptr(), _ld(A, 0, A.shape[1]), B.data_ptr(), _ld(B, 0, N),
           C.data_ptr(), _ld(C, 0, N), M, N, K, alpha, beta),
          "deig_gemm_skinny_workspace", (M, N, K))
    return C
