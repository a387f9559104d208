"""The uint8 centred-PCA kernels through the C ABI: integer column sums (deig_colsum_u8), the
centred exact covariance (deig_syrk_u8_centered) and the fused byte transform
(deig_pca_transform_u8).

References come from the same bytes on the CPU: exact Python / int64 integers for the sums
and the covariance (the rational value for the `center` doubles as given), float64 numpy for
the transform.  All bounds are computed here from the inputs, never from kernel output:
* column sums: raw equal to the integer sum; gray within one rounding (2^-53 relative) of
  sum / 3;
* covariance, the contract of include/deig.h with u = 2^-53, B_ij = (n A_ij - Y_i Y_j) / n and
  e_i = s sum_r (v_ri - c_i):   |S64_ij - exact_ij| <= 8 u (alpha / s^2) (|B_ij| + |e_i e_j| / n),
  tested as an inequality between integers (no rounding in the test itself);
* transform, DESIGN.md §3.4b with u = 2^-24 and t = v - mean in float64:
    |Y - ref| <= (d + 9) u (|t| |W|),  |energy - ref| <= (d + 8) u ref,
    |resid - ||t - W W^T t||^2| <= (d + k + 8) u energy   (orthonormal W).
Harness of every test: rows strided and padded with 0xFF bytes, NaN / sentinel-padded outputs,
a 0xA5 workspace with a canary behind it that is checked after every call.
"""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
CANARY = 1 << 16
FILL = 0xA5
SENTINEL = 777.0
MODES = ["raw", "gray"]


def _lib():
    from distributed_eigenspaces_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Ws:
    """A 0xA5 workspace of exactly nbytes with a canary behind it."""

    def __init__(self, nbytes, cuda):
        self.nbytes = int(nbytes)
        self.t = torch.full((max(self.nbytes, 1) + CANARY,), FILL, dtype=torch.uint8, device=cuda)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert int((self.t[max(self.nbytes, 1):] != FILL).sum()) == 0, "wrote past the workspace"


def _bytes(n, d, mode, seed):
    """Random bytes (n, width), width = d (raw) or 3 d (gray), with a per-column level so that
    the columns' means differ, and the integer features (n, d) int64: x or r + g + b."""
    rng = np.random.default_rng(seed)
    width = d if mode == "raw" else 3 * d
    level = rng.integers(20, 236, size=width)
    x = np.clip(level + np.rint(25.0 * rng.standard_normal((n, width))), 0, 255).astype(np.uint8)
    x[0, :min(4, width)] = (0, 255, 0, 255)[:min(4, width)]  # the extremes occur
    s = x.astype(np.int64)
    if mode == "gray":
        s = s.reshape(n, d, 3).sum(axis=2)
    return x, s


def _strided(x, cuda, pad=4):
    """Rows of x in a device buffer with `pad` 0xFF bytes behind each row."""
    n, w = x.shape
    buf = torch.full((n, w + pad), 0xFF, dtype=torch.uint8, device=cuda)
    buf[:, :w] = torch.from_numpy(x).to(cuda)
    return buf


# ---------------------------------------------------------------- column sums
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [4, 260])
@pytest.mark.parametrize("n", [1, 127, 129, 1000])
def test_column_sums(n, d, mode, cuda):
    L = _lib()
    x, s = _bytes(n, d, mode, 1000 * n + d)
    buf = _strided(x, cuda)
    nbytes = L.lib().deig_colsum_u8_workspace(n, d)
    outs = []
    for _ in range(2):
        sums = torch.full((d + 1,), float("nan"), dtype=torch.float64, device=cuda)
        ws = _Ws(nbytes, cuda)
        rc = L.lib().deig_colsum_u8(buf.data_ptr(), n, d, buf.stride(0), L.U8_MODES[mode],
                                    sums.data_ptr(), ws.ptr(), nbytes, _stream())
        L.check(rc, "deig_colsum_u8")
        ws.check()
        assert bool(torch.isnan(sums[d])), "wrote behind the d sums"
        outs.append(sums[:d].cpu())
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    got = outs[0].numpy()
    tot = s.sum(axis=0)
    if mode == "raw":
        assert np.array_equal(got, tot.astype(np.float64))  # exact integers
    else:
        for j in range(d):
            exact = Fraction(int(tot[j]), 3)
            assert abs(Fraction(float(got[j])) - exact) <= Fraction(1, 2 ** 53) * exact, j
    # the Python wrapper on the column slice of the strided buffer: the same bits
    import distributed_eigenspaces_amd as de
    w = x.shape[1]
    assert torch.equal(de.column_sums_u8(buf[:, :w], mode).cpu(), outs[0])


# ---------------------------------------------------------------- centred covariance
def _scaled_center(c):
    """Doubles c as integers C / 2^q, exactly."""
    fr = [Fraction(float(v)) for v in c]
    q = max(f.denominator.bit_length() - 1 for f in fr)
    return np.array([int(f * (1 << q)) for f in fr], dtype=object), q


def _exact_cov(M, T, n, mode, center, alpha, rows):
    """Rows `rows` of the exact covariance as integers: (num, den) with exact = num / den,
    and the contract's bound as float64.  M = sum s_i s_j and T = sum s_i are the integer
    moments of the features s = x (raw) or r + g + b (gray), v = s / sc; center: doubles in
    units of v or None (the own mean T / (sc n), a rational); alpha: a double."""
    sc = 1 if mode == "raw" else 3
    d = len(T)
    Mo = M[rows].astype(object)
    To = np.array([int(t) for t in T], dtype=object)
    Ti, Tj = To[rows][:, None], To[None, :]
    nB = n * Mo - Ti * Tj  # n B_ij = n M_ij - T_i T_j  (the offset drops out: = n A_ij - Y_i Y_j)
    if center is None:
        q = 0
        ei = np.zeros((len(rows), 1), dtype=object)
        ej = np.zeros((1, d), dtype=object)
    else:
        C, q = _scaled_center(center)
        E = To * (1 << q) - sc * n * C  # e_i 2^q = (T_i - sc n c_i) 2^q
        ei, ej = E[rows][:, None], E[None, :]
    # sc^2 sum (v - c)(v - c)^T = (n B + e_i e_j) / n, over 2^(2 q)
    inner = nB * (1 << (2 * q)) + ei * ej
    fa = Fraction(float(alpha))
    num = inner * fa.numerator
    den = n * (1 << (2 * q)) * sc * sc * fa.denominator
    # 8 u (alpha / sc^2) (|B_ij| + |e_i e_j| / n): Python's int / int is correctly rounded
    mag = np.abs(nB) * (1 << (2 * q)) + np.abs(ei * ej)
    bound = np.array([[(8 * int(m) * fa.numerator) / (den << 53) for m in r] for r in mag])
    return num, den, bound


def _assert_contract(S, num, den, bound, what):
    """|S - num / den| <= bound as an inequality between integers; returns max err / bound."""
    worst = 0.0
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            sp, sq = float(S[i, j]).as_integer_ratio()
            bp, bq = float(bound[i, j]).as_integer_ratio()
            lhs = abs(sp * den - int(num[i, j]) * sq)  # |S - exact| sq den
            # lhs / (sq den) <= bp / bq
            ok = lhs * bq <= bp * sq * den
            if bound[i, j] > 0:
                worst = max(worst, (lhs / (sq * den)) / bound[i, j])
            assert ok, f"{what}: entry ({i}, {j}) off by {lhs / (sq * den):.3e}, bound {bound[i, j]:.3e}"
    return worst


def _run_centered(buf, n, d, mode, center, alpha, cuda, want32=True):
    """One deig_syrk_u8_centered call with S64, S32 and mean_out in NaN-padded storage."""
    L = _lib()
    S64 = torch.full((d, d + 2), float("nan"), dtype=torch.float64, device=cuda)
    S32 = torch.full((d, d + 4), float("nan"), dtype=torch.float32, device=cuda)
    mean = torch.full((d + 1,), float("nan"), dtype=torch.float64, device=cuda)
    c = None if center is None else torch.from_numpy(np.asarray(center, dtype=np.float64)).to(cuda)
    nbytes = L.lib().deig_syrk_u8_centered_workspace(n, d, L.U8_MODES[mode])
    ws = _Ws(nbytes, cuda)
    rc = L.lib().deig_syrk_u8_centered(buf.data_ptr(), n, d, buf.stride(0), L.U8_MODES[mode],
                                       None if c is None else c.data_ptr(), ctypes.c_double(alpha),
                                       S32.data_ptr() if want32 else None, d + 4, S64.data_ptr(),
                                       d + 2, mean.data_ptr(), ws.ptr(), nbytes, _stream())
    L.check(rc, "deig_syrk_u8_centered")
    ws.check()
    assert bool(torch.isnan(S64[:, d:]).all()) and bool(torch.isnan(mean[d])), "wrote into the padding"
    if want32:
        assert bool(torch.isnan(S32[:, d:]).all())
        assert torch.equal(S32[:, :d], S64[:, :d].to(torch.float32)), "S is not S64 rounded to float"
    S = S64[:, :d]
    assert torch.equal(S, S.t()), "not bit-exactly symmetric"
    return S.cpu().numpy(), mean[:d].cpu().numpy()


def _check_mean(mean, T, n, mode):
    sc = 1 if mode == "raw" else 3
    for j, t in enumerate(T):
        exact = Fraction(int(t), sc * n)
        assert abs(Fraction(float(mean[j])) - exact) <= Fraction(2, 2 ** 53) * exact, j


def _pooled(s, mode, seed):
    """The mean (in units of v) of a larger set that the shard is part of."""
    rng = np.random.default_rng(seed)
    extra = np.clip(s.mean(axis=0) + (25.0 if mode == "raw" else 43.0) *
                    rng.standard_normal((50, s.shape[1])), 0, 255 if mode == "raw" else 765)
    return np.concatenate([s.astype(np.float64), np.rint(extra)]).mean(axis=0) / (1 if mode == "raw" else 3)


@pytest.mark.parametrize("center", ["own", "pooled", "zeros"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,d", [(1, 4), (70, 132), (1000, 260)])
def test_centered_covariance_image_path(n, d, mode, center, cuda):
    """Ragged tiles, a ragged last row block, several K segments; every entry against the
    exact rational."""
    import distributed_eigenspaces_amd as de
    x, s = _bytes(n, d, mode, 7 * n + d)
    c = {"own": None, "pooled": _pooled(s, mode, n + d), "zeros": np.zeros(d)}[center]
    alpha = 1.0 / n
    buf = _strided(x, cuda)
    S, mean = _run_centered(buf, n, d, mode, c, alpha, cuda)
    M, T = s.T @ s, s.sum(axis=0)
    num, den, bound = _exact_cov(M, T, n, mode, c, alpha, np.arange(d))
    worst = _assert_contract(S, num, den, bound, f"n={n} d={d} {mode} {center}")
    print(f"u8 centred covariance n={n} d={d} {mode} {center}: worst err / (8 u bound) {worst:.3f}")
    _check_mean(mean, T, n, mode)
    if center == "zeros":
        # the uncentred exact path computes the same matrix with other roundings (not the same
        # bits): the two agree within the same bound
        ref = de.linalg.sigma_hat_u8(buf[:, :x.shape[1]], mode=mode, dtype=torch.float64).cpu().numpy()
        assert np.all(np.abs(S - ref) <= bound)
    # the Python wrapper: the same bits
    Sw, mw = de.sigma_hat_u8_centered(buf[:, :x.shape[1]], None if c is None else torch.from_numpy(c),
                                      mode=mode, return_mean=True)
    assert np.array_equal(Sw.cpu().numpy(), S) and np.array_equal(mw.cpu().numpy(), mean)


@pytest.mark.parametrize("center", ["own", "pooled"])
def test_centered_covariance_direct_epilogue(center, cuda):
    """d = 2048 raw, one K segment: 2 T >= the CU count, so the covariance comes from the
    centred DIRECT epilogue.  Exact check on four rows of every 128-row tile (its edges and
    the wave boundary) against all columns - every tile, both triangles (the mirror stores) -
    and symmetry, padding and the fp32 rounding on the whole matrix."""
    n, d, mode = 70, 2048, "raw"
    x, s = _bytes(n, d, mode, 99)
    c = None if center == "own" else _pooled(s, mode, 5)
    alpha = 1.0 / n
    S, mean = _run_centered(_strided(x, cuda), n, d, mode, c, alpha, cuda)
    rows = np.array(sorted(128 * t + o for t in range(d // 128) for o in (0, 63, 64, 127)))
    M, T = s.T @ s, s.sum(axis=0)
    num, den, bound = _exact_cov(M, T, n, mode, c, alpha, rows)
    worst = _assert_contract(S[rows], num, den, bound, f"direct {center}")
    print(f"u8 centred covariance direct epilogue {center}: worst err / (8 u bound) {worst:.3f}")
    _check_mean(mean, T, n, mode)


@pytest.mark.parametrize("mode", MODES)
def test_shards_about_the_pooled_mean_add_up(mode, cuda):
    """Two shards of unequal size about the pooled mean, weighted n_i / N, add up to the
    own-mean covariance of their concatenation: within the sum of the three calls' bounds
    (plus the two roundings of the weighted sum itself)."""
    n1, n2, d = 700, 300, 132
    N = n1 + n2
    x, s = _bytes(N, d, mode, 31)
    sc = 1 if mode == "raw" else 3
    pooled = s.sum(axis=0) / (sc * N)  # as the all-reduce gives it: one rounding
    buf = _strided(x, cuda)
    Sa, _ = _run_centered(buf, N, d, mode, None, 1.0 / N, cuda)
    S1, _ = _run_centered(buf[:n1], n1, d, mode, pooled, 1.0 / n1, cuda)
    S2, _ = _run_centered(buf[n1:], n2, d, mode, pooled, 1.0 / n2, cuda)
    w1, w2 = n1 / N, n2 / N
    tot = S1 * w1 + S2 * w2
    allr = np.arange(d)
    _, _, ba = _exact_cov(s.T @ s, s.sum(axis=0), N, mode, None, 1.0 / N, allr)
    _, _, b1 = _exact_cov(s[:n1].T @ s[:n1], s[:n1].sum(axis=0), n1, mode, pooled, 1.0 / n1, allr)
    _, _, b2 = _exact_cov(s[n1:].T @ s[n1:], s[n1:].sum(axis=0), n2, mode, pooled, 1.0 / n2, allr)
    # the shards' exact sum about the ROUNDED pooled mean exceeds the own-mean covariance by
    # (mu - pooled)(mu - pooled)^T, |mu - pooled| <= 2^-53 |mu|: far below one unit of the bound
    u = 2.0 ** -53
    mu = np.abs(pooled)
    slack = 3 * u * (np.abs(S1) * w1 + np.abs(S2) * w2) + (u * mu)[:, None] * (u * mu)[None, :]
    err = np.abs(tot - Sa)
    assert np.all(err <= ba + w1 * b1 + w2 * b2 + slack), float(np.max(err))
    own = _run_centered(buf[:n1], n1, d, mode, None, 1.0 / n1, cuda)[0] * w1 + \
        _run_centered(buf[n1:], n2, d, mode, None, 1.0 / n2, cuda)[0] * w2
    assert np.max(np.abs(own - Sa)) > 1e3 * np.max(ba), "the shards' means do not differ"


def test_centered_covariance_large_n_is_exact(cuda):
    """n = 2^25 + 3 raw rows of two patterns at the extremes of the byte range: n A_ii and
    Y_i^2 both exceed 2^63 while their difference is small - the one shape at which an int64
    numerator fails.  The exact answer is closed-form in Python integers."""
    n1, n2, d, mode = 1 << 25, 3, 8, "raw"
    n = n1 + n2
    p1 = np.array([255, 0, 255, 0, 254, 1, 255, 128], dtype=np.int64)
    p2 = np.array([0, 255, 0, 255, 3, 200, 255, 127], dtype=np.int64)
    y1, y2 = p1 - 128, p2 - 128
    A00 = n1 * int(y1[0]) ** 2 + n2 * int(y2[0]) ** 2
    Y0 = n1 * int(y1[0]) + n2 * int(y2[0])
    assert n * A00 > 2 ** 63 and Y0 * Y0 > 2 ** 63  # the int64 numerator's operands overflow
    buf = torch.full((n, d + 4), 0xFF, dtype=torch.uint8, device=cuda)
    buf[:, :d] = torch.from_numpy(p1.astype(np.uint8)).to(cuda)
    where = torch.tensor([5, 1 << 24, n - 1], device=cuda)
    buf[where, :d] = torch.from_numpy(p2.astype(np.uint8)).to(cuda)
    M = np.array([[n1 * int(a) * int(b) + n2 * int(c) * int(e) for a, c in zip(p1, p2)]
                  for b, e in zip(p1, p2)], dtype=object)
    T = np.array([n1 * int(a) + n2 * int(c) for a, c in zip(p1, p2)], dtype=object)
    near = np.array([float(t) / n for t in T]) + np.linspace(-1e-6, 1e-6, d)  # a pooled mean
    for c in (None, near):
        S, mean = _run_centered(buf, n, d, mode, c, 1.0 / n, cuda, want32=False)
        num, den, bound = _exact_cov(M, T, n, mode, c, 1.0 / n, np.arange(d))
        worst = _assert_contract(S, num, den, bound, "large n")
        print(f"u8 centred covariance n = 2^25 + 3, {'own' if c is None else 'near'} centre: "
              f"worst err / (8 u bound) {worst:.3f}; S[0, 0] = {S[0, 0]:.6e}")
        _check_mean(mean, T, n, mode)
    del buf


# ---------------------------------------------------------------- fused byte transform
def _orthonormal(d, k, rng):
    a = rng.standard_normal((d, k)) * np.linspace(1.0, 3.0, k) + np.linspace(0.0, 2.0, d)[:, None]
    return np.linalg.qr(a)[0].astype(np.float32)


class _Case:
    """Bytes, W and mean on the device in strided, padded storage, and the float64 reference."""

    def __init__(self, n, d, k, mode, cuda, centred=True):
        rng = np.random.default_rng(10000 * n + 10 * d + k)
        self.n, self.d, self.k, self.mode, self.cuda = n, d, k, mode, cuda
        self.orth = k <= d
        self.W = _orthonormal(d, k, rng) if self.orth else \
            (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
        self.x, s = _bytes(n, d, mode, 3 * n + d + k)
        self.V = s.astype(np.float64) if mode == "raw" else s.astype(np.float64) / 3.0
        self.mean = None
        if centred:  # one row: its own mean would centre it to zero
            self.mean = self.V.mean(axis=0) if n > 1 else self.V[0] + rng.standard_normal(d)
        self.Xb = _strided(self.x, cuda)
        self.ldw, self.ldy = d + 8, k + 1
        wb = torch.full((k, self.ldw), float("nan"), dtype=torch.float32, device=cuda)
        wb[:, :d] = torch.from_numpy(np.ascontiguousarray(self.W.T)).to(cuda)  # column-major
        self.Wb = wb
        self.mu_dev = None if self.mean is None else torch.from_numpy(self.mean).to(cuda)
        T = self.V - (0.0 if self.mean is None else self.mean)
        W64 = self.W.astype(np.float64)
        self.T, self.W64 = T, W64
        self.Y_ref = T @ W64
        self.Y_bound = (d + 9) * U24 * (np.abs(T) @ np.abs(W64))
        self.en_ref = (T * T).sum(axis=1)
        self.res_ref = ((T - self.Y_ref @ W64.T) ** 2).sum(axis=1)

    def run(self, want=("Y", "resid", "energy")):
        L = _lib()
        n, d, k = self.n, self.d, self.k
        Y = torch.full((n, self.ldy), SENTINEL, dtype=torch.float32, device=self.cuda)
        res = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=self.cuda)
        en = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=self.cuda)
        nbytes = L.lib().deig_pca_transform_u8_workspace(n, d, k)
        ws = _Ws(nbytes, self.cuda)
        rc = L.lib().deig_pca_transform_u8(
            self.Xb.data_ptr(), n, d, self.Xb.stride(0), L.U8_MODES[self.mode],
            None if self.mu_dev is None else self.mu_dev.data_ptr(), self.Wb.data_ptr(), k, self.ldw,
            Y.data_ptr() if "Y" in want else None, self.ldy,
            res.data_ptr() if "resid" in want else None, en.data_ptr() if "energy" in want else None,
            ws.ptr(), nbytes, _stream())
        L.check(rc, "deig_pca_transform_u8")
        ws.check()
        assert bool((Y[:, k] == SENTINEL).all()), "wrote behind the k columns of Y"
        assert float(res[n]) == SENTINEL and float(en[n]) == SENTINEL, "wrote behind the n rows"
        return Y, res[:n], en[:n]

    def check(self, Y, res, en):
        """Every output inside its bound; returns the worst err / bound of each."""
        y = Y[:, :self.k].cpu().numpy().astype(np.float64)
        ey = np.abs(y - self.Y_ref)
        assert np.all(ey <= self.Y_bound), "Y"
        e = en.cpu().numpy().astype(np.float64)
        eb = (self.d + 8) * U24 * self.en_ref
        assert np.all(np.abs(e - self.en_ref) <= eb), "energy"
        r = res.cpu().numpy().astype(np.float64)
        assert np.all(r >= 0)
        rb = (self.d + self.k + 8) * U24 * self.en_ref
        if self.orth:
            assert np.all(np.abs(r - self.res_ref) <= rb), "resid"

        def worst(err, b):
            return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)))
        return (worst(ey, self.Y_bound), worst(np.abs(e - self.en_ref), eb),
                worst(np.abs(r - self.res_ref), rb) if self.orth else 0.0)


TRANSFORM_CASES = [("raw", 1, 4, 1), ("raw", 65, 36, 3), ("raw", 129, 260, 17), ("raw", 70, 64, 64),
                   ("raw", 64, 32, 256), ("gray", 65, 36, 3), ("gray", 129, 260, 17)]


@pytest.mark.parametrize("centred", [True, False], ids=["mean", "nomean"])
@pytest.mark.parametrize("mode,n,d,k", TRANSFORM_CASES)
def test_transform(mode, n, d, k, centred, cuda):
    """Row-tile tails, super-chunk tails (d = 4, 36, 260: 1, 4 and 1 compute chunks in the
    last one), k < kp and every fragment count class, both modes; repeats give the same
    bits; the float kernel on the widened samples agrees within the sum of both bounds."""
    import distributed_eigenspaces_amd as de
    c = _Case(n, d, k, mode, cuda, centred)
    Y, res, en = c.run()
    w = c.check(Y, res, en)
    print(f"pca_transform_u8 {mode} n={n} d={d} k={k} {'mean' if centred else 'no mean'}: "
          f"worst err / bound Y {w[0]:.4f} energy {w[1]:.4f} resid {w[2]:.4f}")
    Y2, res2, en2 = c.run()
    assert torch.equal(Y, Y2) and torch.equal(res, res2) and torch.equal(en, en2)
    # today's route: widen, then pca_transform (raw widens exactly; gray is widened to float64,
    # which pca_transform centres in float64 and rounds once, the same t as here)
    Xw = torch.from_numpy(c.V.astype(np.float32) if mode == "raw" else c.V).to(cuda)
    Yf = de.pca_transform(Xw, torch.from_numpy(c.W).to(cuda),
                          None if c.mean is None else torch.from_numpy(c.mean))
    diff = np.abs(Yf.cpu().numpy().astype(np.float64) - Y[:, :k].cpu().numpy().astype(np.float64))
    assert np.all(diff <= 2 * c.Y_bound)
    # and the Python wrapper gives the kernel's bits
    Yw, rw, ew = de.pca_transform_u8(c.Xb[:, :c.x.shape[1]], torch.from_numpy(c.W).to(cuda),
                                     None if c.mean is None else torch.from_numpy(c.mean), mode,
                                     residual=True, energy=True)
    assert torch.equal(Yw, Y[:, :k]) and torch.equal(rw, res) and torch.equal(ew, en)


def test_transform_every_combination_of_outputs(cuda):
    c = _Case(129, 260, 17, "gray", cuda)
    Y, res, en = c.run()
    c.check(Y, res, en)
    names = ("Y", "resid", "energy")
    for r in (1, 2):
        for want in itertools.combinations(names, r):
            Y1, res1, en1 = c.run(want)
            assert torch.equal(Y1, Y) if "Y" in want else bool((Y1 == SENTINEL).all()), want
            assert torch.equal(res1, res) if "resid" in want else bool((res1 == SENTINEL).all()), want
            assert torch.equal(en1, en) if "energy" in want else bool((en1 == SENTINEL).all()), want


def test_transform_wrapper_pads_features(cuda):
    """d % 4 != 0 through the wrapper: zero bytes, zero rows of W, zero mean entries."""
    import distributed_eigenspaces_amd as de
    for mode, d in (("raw", 37), ("gray", 9)):
        n, k = 70, 5
        x, s = _bytes(n, d, mode, 17)
        V = s.astype(np.float64) / (1 if mode == "raw" else 3)
        mu = V.mean(axis=0)
        W = _orthonormal(d, k, np.random.default_rng(3))
        xt = torch.from_numpy(x).to(cuda)
        Y, res, en = de.pca_transform_u8(xt, torch.from_numpy(W).to(cuda), torch.from_numpy(mu), mode,
                                         residual=True, energy=True)
        T, W64 = V - mu, W.astype(np.float64)
        ref = T @ W64
        assert np.all(np.abs(Y.cpu().numpy() - ref) <= (d + 9) * U24 * (np.abs(T) @ np.abs(W64)))
        e_ref = (T * T).sum(axis=1)
        assert np.all(np.abs(en.cpu().numpy() - e_ref) <= (d + 8) * U24 * e_ref)
        r_ref = ((T - ref @ W64.T) ** 2).sum(axis=1)
        assert np.all(np.abs(res.cpu().numpy() - r_ref) <= (d + k + 8) * U24 * e_ref)
        # the padded covariance and sums crop back to d
        S, m = de.sigma_hat_u8_centered(xt, mode=mode, return_mean=True)
        assert S.shape == (d, d) and m.shape == (d,)
        np.testing.assert_allclose(m.cpu().numpy(), mu, rtol=1e-15)
        np.testing.assert_allclose(S.cpu().numpy(), T.T @ T / n, rtol=1e-12, atol=1e-12 * np.max(T * T))
        np.testing.assert_allclose(de.column_sums_u8(xt, mode).cpu().numpy(), V.sum(axis=0), rtol=1e-15)


def test_transform_short_workspace_is_reported_and_outputs_untouched(cuda):
    L = _lib()
    c = _Case(65, 36, 3, "raw", cuda)
    nbytes = L.lib().deig_pca_transform_u8_workspace(65, 36, 3)
    ws = _Ws(nbytes, cuda)
    Y = torch.full((65, 4), SENTINEL, dtype=torch.float32, device=cuda)
    rc = L.lib().deig_pca_transform_u8(c.Xb.data_ptr(), 65, 36, c.Xb.stride(0), L.DEIG_U8_RAW, None,
                                       c.Wb.data_ptr(), 3, c.ldw, Y.data_ptr(), 4, None, None,
                                       ws.ptr(), nbytes - 1, _stream())
    assert rc == L.DEIG_EWORKSPACE and "workspace" in L.last_error()
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all()) and bool((ws.t == FILL).all()), "GPU work before the check"
