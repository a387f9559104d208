"""The covariance of bf16 samples taken as they are (deig_syrk_bf16, ``sigma_hat`` on
``torch.bfloat16``) against float64 / int64 references computed from the bf16 values.

* Exact cases: integer entries in [-15, 15] are exact in bf16 and every partial sum of their
  products is an integer below 2^24 (n <= 74565), so S must EQUAL the int64 reference in any
  summation order - through a NaN-poisoned workspace, a NaN-filled S and a row stride whose
  tail columns hold NaN.
* Rounded data: every product is exact, the error is the two-level fp32 summation alone:
  max |S - S_ref| <= 2e-6 max |S_ref| (the project's SYRK bar, tests/test_gpu_syrk_chunks.py;
  the model (16384 / 32 + n / 16384) eps puts the expectation near 5e-7), bit symmetry and
  bit-identical repeats.
* No fp32 copy: the peak of the allocator rises by less than the shard's fp32 size.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 2e-6


def _lib():
    from distributed_eigenspaces_amd import _lib as L
    return L


def _int_samples(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-15, 16, size=(n, d), dtype=np.int64)


def _gram(xi):
    """xi^T xi as int64: formed in float64, exact (every partial sum is an integer < 2^53)."""
    x = xi.astype(np.float64)
    return (x.T @ x).astype(np.int64)


def _strided_bf16(xi, pad, cuda):
    """The integer samples as bf16 rows with ``pad`` NaN elements behind each row."""
    n, d = xi.shape
    buf = torch.full((n, d + pad), float("nan"), dtype=torch.bfloat16, device=cuda)
    buf[:, :d] = torch.from_numpy(xi.astype(np.float32)).to(cuda).to(torch.bfloat16)
    return buf


def _raw(buf, n, d, alpha, S, flags, ws, nbytes):
    L = _lib()
    return L.lib().deig_syrk_bf16(buf.data_ptr(), n, d, buf.stride(0), ctypes.c_float(alpha),
                                  S.data_ptr(), S.stride(0), flags,
                                  ws.data_ptr() if ws is not None else None, nbytes,
                                  torch.cuda.current_stream().cuda_stream)


def _poisoned(nbytes, cuda):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=cuda)  # every float a NaN


@pytest.mark.parametrize("n,d", [(1, 8), (31, 8), (33, 136), (1000, 264), (4099, 520)])
def test_exact_on_integer_data(n, d, cuda):
    L = _lib()
    xi = _int_samples(n, d, seed=100 * n + d)
    ref = _gram(xi)
    assert np.abs(ref).max() < 2 ** 24
    buf = _strided_bf16(xi, 8, cuda)
    S = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    nbytes = L.lib().deig_syrk_bf16_workspace(n, d)
    ws = _poisoned(nbytes, cuda)
    L.check(_raw(buf, n, d, 1.0, S, 0, ws, nbytes), "deig_syrk_bf16")
    torch.cuda.synchronize()
    got = S.cpu().numpy()
    assert np.array_equal(got.astype(np.int64), ref) and np.array_equal(got, ref.astype(np.float32))
    # the wrapper on a column slice of the strided buffer: the same bits
    import distributed_eigenspaces_amd as de
    assert torch.equal(de.sigma_hat(buf[:, :d], alpha=1.0), S)


@pytest.mark.parametrize("d", [136, 520])
def test_exact_with_a_power_of_two_alpha(d, cuda):
    L = _lib()
    n = 1024
    xi = _int_samples(n, d, seed=d)
    ref = _gram(xi).astype(np.float64) / 1024.0  # exact in fp32: integers below 2^24 / 2^10
    buf = _strided_bf16(xi, 8, cuda)
    S = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    nbytes = L.lib().deig_syrk_bf16_workspace(n, d)
    L.check(_raw(buf, n, d, 1.0 / 1024, S, 0, _poisoned(nbytes, cuda), nbytes), "deig_syrk_bf16")
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy().astype(np.float64), ref)
    import distributed_eigenspaces_amd as de
    assert torch.equal(de.sigma_hat(buf[:, :d]), S)  # alpha = 1 / n by default


def test_row_chunks_from_a_small_workspace(cuda):
    """n = 16359 rows through a workspace sized for 4096: 4 chunks (the last one partial)
    accumulating into S; integer data, so the result is still exact."""
    L = _lib()
    n, d, chunk = 16359, 520, 4096
    xi = _int_samples(n, d, seed=7)
    ref = _gram(xi)
    assert np.abs(ref).max() < 2 ** 24
    buf = _strided_bf16(xi, 8, cuda)
    nbytes = L.lib().deig_syrk_bf16_workspace(chunk, d)
    assert nbytes < L.lib().deig_syrk_bf16_workspace(n, d), "one chunk would hold all rows"
    S = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    L.check(_raw(buf, n, d, 1.0, S, 0, _poisoned(nbytes, cuda), nbytes), "deig_syrk_bf16")
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy().astype(np.int64), ref)
    # the same rows with the recommended workspace: the same (exact) result
    nb1 = L.lib().deig_syrk_bf16_workspace(n, d)
    S1 = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    L.check(_raw(buf, n, d, 1.0, S1, 0, _poisoned(nb1, cuda), nb1), "deig_syrk_bf16")
    torch.cuda.synchronize()
    assert torch.equal(S1, S)
    # below the one-chunk minimum: an error, and S is not touched
    least = L.lib().deig_syrk_bf16_workspace(1, d)
    S2 = torch.full((d, d), 5.0, dtype=torch.float32, device=cuda)
    assert _raw(buf, n, d, 1.0, S2, 0, _poisoned(least, cuda), least - 1) == L.DEIG_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((S2 == 5.0).all())


@pytest.mark.parametrize("d", [264, 520])
def test_accumulate_row_blocks(d, cuda):
    """Four ragged row blocks through sigma_hat(..., out=S, accumulate=True) with alpha = 1 / N,
    N a power of two: integer data, exact."""
    import distributed_eigenspaces_amd as de
    sizes = [1000, 1031, 997, 1068]
    N = sum(sizes)
    assert N == 4096
    xi = _int_samples(N, d, seed=3 * d + 1)
    ref = _gram(xi).astype(np.float64) / N
    x = torch.from_numpy(xi.astype(np.float32)).to(cuda).to(torch.bfloat16)
    bounds = np.cumsum([0] + sizes)
    S = torch.zeros((d, d), dtype=torch.float32, device=cuda)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        out = de.sigma_hat(x[lo:hi], alpha=1.0 / N, out=S, accumulate=True)
        assert out is S
    torch.cuda.synchronize()
    assert np.array_equal(S.cpu().numpy().astype(np.float64), ref)
    # the first block without accumulate overwrites whatever S held
    S2 = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        de.sigma_hat(x[lo:hi], alpha=1.0 / N, out=S2, accumulate=i > 0)
    assert torch.equal(S2, S)
    with pytest.raises(ValueError):
        de.sigma_hat(x[:100], accumulate=True)  # no out


@pytest.mark.parametrize("n,d", [(16384, 1024), (262144, 256)])
def test_rounded_data_meets_the_syrk_bar(n, d, cuda):
    import distributed_eigenspaces_amd as de
    g = torch.Generator(device="cpu").manual_seed(n + d)
    x = (3.0 * torch.randn((n, d), generator=g) + 1.0).to(torch.bfloat16)
    x64 = x.double()
    ref = (x64.t() @ x64 / n).numpy()
    xg = x.to(cuda)
    S = de.sigma_hat(xg)
    assert S.dtype == torch.float32 and S.shape == (d, d)
    assert torch.equal(S, S.t()), "S must be bit-exactly symmetric"
    assert torch.equal(S, de.sigma_hat(xg)), "repeated calls must give identical bits"
    err = np.abs(S.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"bf16 syrk n={n} d={d}: max |S - S_ref| / max |S_ref| = {err:.3e} (bar {REL:.0e})")
    assert err <= REL


def test_no_fp32_copy_of_the_samples(cuda):
    import distributed_eigenspaces_amd as de
    n, d = 16384, 2048
    x = torch.randn((n, d), device=cuda).to(torch.bfloat16)
    de.sigma_hat(x[:64])  # the library is loaded and warm
    torch.cuda.synchronize()
    from distributed_eigenspaces_amd import linalg
    linalg._ws.bufs.clear()  # the cached workspace counts as part of the call
    before = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    S = de.sigma_hat(x)
    torch.cuda.synchronize()
    after = torch.cuda.max_memory_allocated()
    rise = after - base
    print(f"peak before reset {before}, at reset {base}, after sigma_hat {after}: rise {rise} "
          f"bytes, fp32 copy {n * d * 4}")
    assert rise < n * d * 4 and after - before < n * d * 4
    assert S.shape == (d, d)
