"""The K loop that the uint8 and bf16 covariance kernels share (csrc/syrk_image_tile.hpp) at
every tail length of its register ring, on exact integer data: a stage that is skipped, run
twice or read from the wrong ring slot changes an integer sum.

The ring holds PF stages (bf16: PF = 2, a stage = 64 rows; uint8: PF = 4, a stage = 64 rows),
and a segment of m stages runs m / PF unrolled rounds and a tail of m % PF, so the segment
lengths 1 .. 2 PF + 1 take every path: shorter than the ring, one round, a round and each
tail, two rounds, two rounds and a tail.  The shapes below give one known length per segment:

* bf16, d = 136 (fpad = 256: T = 3 lower tiles, two diagonal and one off-diagonal),
  n = 64 m - 5, m = 1 .. 7.  syrk_bf16_launch: nst = cdiv(n, 64) = m; nseg = cdiv(512, T) = 171,
  cut to max_segs = 32, then to nst / 4 <= 1 (m < 8), then raised to cdiv(nst, 256) = 1: one
  segment of m stages.  Entries are integers in [-15, 15]: exact in bf16, every partial sum an
  integer below 2^24, so S must EQUAL the int64 Gram.
* uint8 raw, d = 260 (fpad = 384: T = 6 tiles), n = 64 m - 3, m = 1 .. 4.  u8_run: nkb = m;
  2 T = 12 < CUs, so the image path (atomic epilogue); nseg = cdiv(2 CUs, T) is cut to
  cdiv(nkb, 4) = 1: one segment of m K-steps.
* uint8 raw, d = 1024 (T = 36 tiles), n = 64 nseg L - 3, L = 5 .. 9, nseg = cdiv(2 CUs, 36)
  (15 on 256 CUs): 2 T = 72 < CUs, so the image path; nkb = nseg L, nseg <= cdiv(nkb, 4), and
  segment s is the K-steps nkb s / nseg = L s .. L (s + 1) - 1: every segment has L K-steps.
  Needs more than 72 CUs (else the direct path runs, one segment of all K-steps).
* The direct epilogue's K loop is the same code; tests/test_gpu_u8.py
  test_direct_epilogue_edges runs it over 47 and 1024 K-steps.

The uint8 result is taken in float64 with alpha = 1 / n: the library rounds the exact
integer sum's quotient by n once, and so does the reference (the int64 Gram, formed in
float64 on the host where every partial sum is an integer below 2^53, divided by n): the two
may differ by the rounding of one IEEE division at most, rtol = 2^-52.  Workspace and S are
NaN-poisoned first."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from distributed_eigenspaces_amd import _lib as L
    return L


def _gram(x):
    """x^T x as int64: formed in float64, exact (every partial sum is an integer < 2^53)."""
    xf = x.astype(np.float64)
    return (xf.T @ xf).astype(np.int64)


def _poisoned(nbytes, cuda):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=cuda)  # every float a NaN


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7])
def test_bf16_segment_of_m_stages(m, cuda):
    L = _lib()
    n, d = 64 * m - 5, 136
    xi = np.random.default_rng(m).integers(-15, 16, size=(n, d), dtype=np.int64)
    ref = _gram(xi)
    assert np.abs(ref).max() < 2 ** 24
    x = torch.from_numpy(xi.astype(np.float32)).to(cuda).to(torch.bfloat16)
    S = torch.full((d, d), float("nan"), dtype=torch.float32, device=cuda)
    nbytes = L.lib().deig_syrk_bf16_workspace(n, d)
    ws = _poisoned(nbytes, cuda)
    L.check(L.lib().deig_syrk_bf16(x.data_ptr(), n, d, x.stride(0), ctypes.c_float(1.0), S.data_ptr(),
                                   S.stride(0), 0, ws.data_ptr(), nbytes,
                                   torch.cuda.current_stream().cuda_stream), "deig_syrk_bf16")
    torch.cuda.synchronize()
    got = S.cpu().numpy()
    assert np.array_equal(got, ref.astype(np.float32)) and np.array_equal(got.astype(np.int64), ref)


def _u8_cov64(X, cuda):
    """deig_syrk_u8 (raw, alpha = 1 / n, float64 result) through a poisoned workspace and S."""
    L = _lib()
    n, d = X.shape
    x = torch.from_numpy(X).to(cuda)
    S = torch.full((d, d), float("nan"), dtype=torch.float64, device=cuda)
    nbytes = L.lib().deig_syrk_u8_workspace(n, d, L.DEIG_U8_RAW)
    ws = _poisoned(nbytes, cuda)
    L.check(L.lib().deig_syrk_u8(x.data_ptr(), n, d, x.stride(0), L.DEIG_U8_RAW, 1.0 / n, None, d,
                                 S.data_ptr(), S.stride(0), ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream), "deig_syrk_u8")
    torch.cuda.synchronize()
    return S.cpu().numpy()


def _check_u8(got, gram, n):
    want = gram.astype(np.float64) / n
    rel = np.abs(got - want) / want  # (want > 0: sums of products of bytes, none all zero)
    print(f"n={n} d={got.shape[0]}: max rel. difference to the exact quotient {rel.max():.3e}")
    assert np.isfinite(got).all() and rel.max() <= 2.0 ** -52
    assert np.array_equal(got, got.T)


def _cus(cuda):
    return torch.cuda.get_device_properties(cuda).multi_processor_count


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_u8_one_segment_of_m_ksteps(m, cuda):
    if _cus(cuda) <= 12:
        pytest.skip("2 T = 12 >= CUs: the direct path would run")
    n, d = 64 * m - 3, 260
    X = np.random.default_rng(10 + m).integers(1, 256, (n, d), dtype=np.uint8)
    _check_u8(_u8_cov64(X, cuda), _gram(X), n)


LENGTHS = (5, 6, 7, 8, 9)


@functools.lru_cache(maxsize=1)
def _long_cases(nseg):
    """The samples of the longest case and the Gram of each case's leading rows (one pass)."""
    ns = [64 * nseg * L - 3 for L in LENGTHS]
    X = np.random.default_rng(99).integers(1, 256, (ns[-1], 1024), dtype=np.uint8)
    grams, g, lo = {}, np.zeros((1024, 1024), dtype=np.int64), 0
    for L, n in zip(LENGTHS, ns):
        g = g + _gram(X[lo:n])
        grams[L], lo = g, n
    return X, grams


@pytest.mark.parametrize("L", LENGTHS)
def test_u8_segments_of_L_ksteps(L, cuda):
    cus = _cus(cuda)
    if cus <= 72:
        pytest.skip("2 T = 72 >= CUs: the direct path would run, one segment of all K-steps")
    nseg = -(-2 * cus // 36)
    n = 64 * nseg * L - 3
    X, grams = _long_cases(nseg)
    _check_u8(_u8_cov64(X[:n], cuda), grams[L], n)
