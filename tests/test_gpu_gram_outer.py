"""The sample-space Gram matrix of the wide-data route, K = alpha Xc Xc^T (linalg.gram_outer,
deig_gram_outer), on float32, bfloat16 and uint8 rows.

Every product the bf16 MFMA forms is exact in fp32; the errors are the dropped terms of the
hi / lo split and the fp32 summation.  With u = 2^-24, gamma_m = m u / (1 - m u) and T the
staged matrix fl32((double)x - c), element by element:
  uncentred bf16 / uint8 (and float32 values that are bf16 values): exact while every
      sum_f |t_if t_jf| < 2^24 and alpha is a power of two;
  float32 samples and all centred calls:
      |K - K64| <= (2^-16 + 1.01 gamma_3d + 2 u) alpha (|T| |T|^T).
The reference is float64 NumPy on T, never another GPU route."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.golden_data import spiked_int_data

pytestmark = pytest.mark.gpu
KINDS = ("f32", "bf16", "u8")
U = 2.0 ** -24


def _gamma(m):
    return m * U / (1 - m * U)


def _bound(d):
    return 2.0 ** -16 + 1.01 * _gamma(3 * d) + 2 * U


def _staged(x: torch.Tensor, c):
    """Xc as float64 NumPy: what the kernels stage."""
    x64 = x.cpu().to(torch.float64)
    if c is None:
        return x64.numpy()
    return (x64 - torch.as_tensor(c, dtype=torch.float64)).to(torch.float32).to(torch.float64).numpy()


def _as_kind(a: np.ndarray, kind, dev):
    """Integers 0..255 as samples of the kind (all three hold them exactly)."""
    if kind == "u8":
        return torch.from_numpy(a.astype(np.uint8)).to(dev)
    t = torch.from_numpy(a.astype(np.float32)).to(dev)
    return t.to(torch.bfloat16) if kind == "bf16" else t


INT_SHAPES = [(40, 136, 255), (200, 136, 255), (384, 1032, 100), (130, 16424, 15)]


@functools.lru_cache(maxsize=None)
def _int_inputs(n, d, hi):
    a = np.random.default_rng(1000 * n + d).integers(0, hi + 1, size=(n, d)).astype(np.int64)
    K = a @ a.T
    assert K.max() < 2 ** 24  # every sum |x_i x_j| stays an exact fp32 integer
    return a, K


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hi", INT_SHAPES)
def test_exact_on_integers(n, d, hi, kind, cuda):
    import distributed_eigenspaces_amd as de
    a, K64 = _int_inputs(n, d, hi)
    K = de.gram_outer(_as_kind(a, kind, cuda), alpha=1.0)
    assert K.shape == (n, n) and K.dtype == torch.float32
    assert torch.equal(K.cpu().to(torch.int64), torch.from_numpy(K64))


def _forms(Xq, dev):
    return {"u8": torch.from_numpy((Xq + 128).astype(np.uint8)).to(dev),
            "f32": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev),
            "bf16": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev).to(torch.bfloat16)}


CENTRED_SHAPES = [(200, 136), (384, 1032)]


@functools.lru_cache(maxsize=None)
def _centred_inputs(n, d):
    Xq, _ = spiked_int_data(n, d, 4, seed=100 + n)
    assert Xq.min() >= -128 and Xq.max() <= 127  # none clip
    return Xq


@functools.lru_cache(maxsize=None)
def _centred_reference(n, d, kind, which):
    """(centre, K64, |T||T|^T / n) about the column mean or an arbitrary other vector."""
    x = _forms(_centred_inputs(n, d), "cpu")[kind]
    c = x.to(torch.float64).mean(dim=0)
    if which == "other":
        c = c * 0.75 + torch.from_numpy(np.random.default_rng(d).standard_normal(d)) * 0.3
    T = _staged(x, c)
    return c, T @ T.T / n, np.abs(T) @ np.abs(T).T / n


def _assert_bound(K, K64, A, d, what):
    err = np.abs(K.cpu().to(torch.float64).numpy() - K64)
    ratio = float(np.max(err / A))
    print(f"{what}: max |K - K64| / (alpha |T||T|^T) = {ratio:.3e}, bound {_bound(d):.3e}")
    assert np.all(err <= _bound(d) * A)


@pytest.mark.parametrize("which", ("mean", "other"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", CENTRED_SHAPES)
def test_centred_bound(n, d, kind, which, cuda):
    import distributed_eigenspaces_amd as de
    x = _forms(_centred_inputs(n, d), cuda)[kind]
    c, K64, A = _centred_reference(n, d, kind, which)
    _assert_bound(de.gram_outer(x, center=c), K64, A, d, f"{kind} {n}x{d} about the {which}")


@pytest.mark.parametrize("centred", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_outside_is_read(kind, centred, cuda):
    """X as the [:n, :d] view of a larger tensor whose other entries are NaN (255 for bytes)."""
    import distributed_eigenspaces_amd as de
    n, d = 200, 136
    x = _forms(_centred_inputs(n, d), cuda)[kind]
    big = torch.full((n + 8, d + 24), 255 if kind == "u8" else float("nan"), dtype=x.dtype, device=cuda)
    big[:n, :d] = x
    view = big[:n, :d]
    assert view.data_ptr() == big.data_ptr() and view.stride(0) == d + 24
    c = _centred_reference(n, d, kind, "mean")[0] if centred else None
    K = de.gram_outer(view, center=c)
    assert torch.isfinite(K).all()
    assert torch.equal(K, de.gram_outer(x.contiguous(), center=c))


@pytest.mark.parametrize("kind", KINDS)
def test_symmetric_and_deterministic(kind, cuda):
    import distributed_eigenspaces_amd as de
    n, d = 384, 1032
    x = _forms(_centred_inputs(n, d), cuda)[kind]
    for c in (None, _centred_reference(n, d, kind, "mean")[0]):
        K = de.gram_outer(x, center=c)
        assert torch.equal(K, K.t())
        assert torch.equal(K, de.gram_outer(x, center=c))


def _raw_call(x, c, alpha, ws_bytes, cuda):
    """deig_gram_outer on a workspace of exactly ws_bytes bytes, filled with NaN bit patterns."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    xt = {torch.float32: _lib.DEIG_F32, torch.bfloat16: _lib.DEIG_BF16, torch.uint8: _lib.DEIG_U8}[x.dtype]
    n, d = x.shape
    K = torch.full((n, n), float("nan"), dtype=torch.float32, device=cuda)
    ws = torch.full((max(ws_bytes, 16),), 0xFF, dtype=torch.uint8, device=cuda)
    cd = None if c is None else c.to(cuda)
    rc = L.deig_gram_outer(x.data_ptr(), xt, n, d, x.stride(0), None if cd is None else cd.data_ptr(),
                           ctypes.c_float(alpha), K.data_ptr(), n, 0, ws.data_ptr(), ws_bytes,
                           torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    return rc, K, xt


@pytest.mark.parametrize("kind", KINDS)
def test_feature_chunks(kind, cuda):
    """A workspace of query(n, d / 4) bytes runs the product in four feature chunks."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    n, d = 384, 1032
    dq = -(-(d // 4) // 8) * 8  # d / 4 rounded to the widest load group
    a, K64 = _int_inputs(n, d, 100)
    x = _as_kind(a, kind, cuda)
    xt = {"f32": _lib.DEIG_F32, "bf16": _lib.DEIG_BF16, "u8": _lib.DEIG_U8}[kind]
    small, full = L.deig_gram_outer_workspace(n, dq, xt, 0), L.deig_gram_outer_workspace(n, d, xt, 0)
    assert 0 < small < full
    rc, K, _ = _raw_call(x, None, 1.0, small, cuda)
    assert rc == _lib.DEIG_OK
    assert torch.equal(K.cpu().to(torch.int64), torch.from_numpy(K64))

    x = _forms(_centred_inputs(n, d), cuda)[kind]
    c, Kc64, A = _centred_reference(n, d, kind, "mean")
    small = L.deig_gram_outer_workspace(n, dq, xt, 1)
    assert 0 < small < L.deig_gram_outer_workspace(n, d, xt, 1)
    rc, K, _ = _raw_call(x, c, 1.0 / n, small, cuda)
    assert rc == _lib.DEIG_OK
    assert torch.equal(K, K.t())
    _assert_bound(K, Kc64, A, d, f"{kind} {n}x{d} in chunks")

    least = L.deig_gram_outer_workspace(n, 16, xt, 1)
    assert 0 < least <= small
    rc, _, _ = _raw_call(x, c, 1.0 / n, least - 1, cuda)
    assert rc == _lib.DEIG_EWORKSPACE
