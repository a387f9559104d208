"""The centred-PCA kernels against float64 numpy of the same inputs: column sums
(deig_colsum), the centred covariance (deig_syrk_centered) and the fused centred transform
(deig_pca_transform_f32), each through the C ABI with strided, NaN-padded storage.

Bounds (all computed here from the shapes, none from what the kernels give):
* column sums: n 2^-52 sum_r |x_rj| (a double sum of n terms in any order);
* covariance: 1e-5 max|cov about the shard's own mean| + 1e-12 max|ref| - the bar
  tests/test_gpu_f64flow.py applies to the same SYRK (fp32-grade on the centred scale, the
  mean terms in double);
* transform, with u = 2^-24 and t = x - mean in float64:
    |Y - ref|      <= (d + 9) u (|t| |W|)   the fp32 dot-product model of
                      tests/test_gpu_skinny.py's ``project`` plus one rounding of t;
    |energy - ref| <= (d + 8) u ref          (one rounding of t doubled by the square, then
                      a sum of d non-negative terms);
    |resid - ||t - W W^T t||^2| <= (d + k + 8) u energy   (both norms, k terms more).
  The mean must be subtracted BEFORE the product for the first one: at mean 1000, spread 1
  the post-hoc form X W - mean^T W misses it by more than 10x (checked here on the CPU in
  an fp32 emulation of both forms, beside the kernel).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = 1 << 16
FILL = 0xA5
SENTINEL = 777.0


def _lib():
    from distributed_eigenspaces_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes, cuda, canary=0):
    return torch.full((max(int(nbytes), 1) + canary,), FILL, dtype=torch.uint8, device=cuda)


def _padded(a, pad, cuda):
    """Rows of ``a`` in a buffer with ``pad`` NaN elements behind each row."""
    n, d = a.shape
    buf = torch.full((n, d + pad), float("nan"), dtype=torch.from_numpy(a[:0]).dtype, device=cuda)
    buf[:, :d] = torch.from_numpy(a).to(cuda)
    return buf


# ---------------------------------------------------------------- column sums
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 4, 257])
@pytest.mark.parametrize("n", [1, 127, 129, 1000])
def test_column_sums(n, d, dtype, cuda):
    L = _lib()
    rng = np.random.default_rng(1000 * n + d)
    x = (50.0 + 20.0 * rng.standard_normal((n, d))).astype(dtype)
    buf = _padded(x, 4, cuda)
    sums = torch.full((d,), float("nan"), dtype=torch.float64, device=cuda)
    nbytes = L.lib().deig_colsum_workspace(n, d)
    ws = _ws(nbytes, cuda, CANARY)
    xtype = L.DEIG_F64 if dtype == np.float64 else L.DEIG_F32
    rc = L.lib().deig_colsum(buf.data_ptr(), xtype, n, d, d + 4, sums.data_ptr(), ws.data_ptr(),
                             nbytes, _stream())
    L.check(rc, "deig_colsum")
    torch.cuda.synchronize()
    assert int((ws[nbytes:] != FILL).sum()) == 0, "wrote past the workspace"
    x64 = x.astype(np.float64)
    err = np.abs(sums.cpu().numpy() - x64.sum(axis=0))
    bound = n * 2.0 ** -52 * np.abs(x64).sum(axis=0)
    assert np.all(err <= bound), f"max err / bound = {np.max(err / bound):.3f}"
    # the Python wrapper on a column slice of the padded buffer, twice: the same bits
    import distributed_eigenspaces_amd as de
    s1, s2 = de.column_sums(buf[:, :d]), de.column_sums(buf[:, :d])
    assert torch.equal(s1, sums) and torch.equal(s1, s2)


# ---------------------------------------------------------------- centred covariance
COV_SHAPES = [(1, 4), (100, 37), (1000, 256), (4099, 520)]


def _cov_data(n, d, extra=50):
    """A shard of n rows out of a larger set (whose mean is the 'pooled' centre)."""
    rng = np.random.default_rng(7 * n + d)
    allx = (100.0 + 20.0 * rng.standard_normal((n + extra, d))).astype(np.float32)
    return allx[:n], allx.astype(np.float64).mean(axis=0)


def _cov_ref(x, c):
    t = x.astype(np.float64) - c
    return t.T @ t / x.shape[0]


def _cov_bar(x, ref):
    own = _cov_ref(x, x.astype(np.float64).mean(axis=0))
    return 1e-5 * np.max(np.abs(own)) + 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("center", ["own", "pooled", "zeros"])
@pytest.mark.parametrize("n,d", COV_SHAPES)
def test_centered_covariance(n, d, center, cuda):
    import distributed_eigenspaces_amd as de
    x, pooled = _cov_data(n, d)
    own = x.astype(np.float64).mean(axis=0)
    c = {"own": None, "pooled": pooled, "zeros": np.zeros(d)}[center]
    xt = torch.from_numpy(x).to(cuda)
    S, mean = de.sigma_hat_centered(xt, None if c is None else torch.from_numpy(c), return_mean=True)
    assert S.dtype == torch.float64 and S.shape == (d, d)
    assert torch.equal(S, S.t()), "not bit-exactly symmetric"
    ref = _cov_ref(x, own if c is None else c)
    err = np.max(np.abs(S.cpu().numpy() - ref))
    bar = _cov_bar(x, ref)
    print(f"centred covariance n={n} d={d} {center}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    np.testing.assert_allclose(mean.cpu().numpy(), own, rtol=1e-14)
    # the float32 output is the rounding of the float64 one
    S32 = de.sigma_hat_centered(xt, None if c is None else torch.from_numpy(c), dtype=torch.float32)
    assert torch.equal(S32, S.to(torch.float32))
    if center == "zeros":  # deig_syrk_shift is exactly this case
        assert torch.equal(S, de.linalg.sigma_hat_shift(xt))
        assert torch.equal(S32, de.linalg.sigma_hat_shift(xt, dtype=torch.float32))


def test_centered_covariance_float64_samples(cuda):
    import distributed_eigenspaces_amd as de
    x, pooled = _cov_data(100, 37)
    x64 = x.astype(np.float64) + 1e-9  # not representable in float32
    S = de.sigma_hat_centered(torch.from_numpy(x64).to(cuda), torch.from_numpy(pooled))
    t = x64 - pooled
    ref = t.T @ t / 100
    assert np.max(np.abs(S.cpu().numpy() - ref)) <= _cov_bar(x64, ref)
    assert torch.equal(S, S.t())


def test_shards_about_the_pooled_mean_add_up(cuda):
    """Two shards of unequal size (one on each side of the split3 threshold), each centred
    about the pooled mean and weighted n_i / N, sum to the pooled centred covariance;
    centred about their own means they do not."""
    import distributed_eigenspaces_amd as de
    rng = np.random.default_rng(5)
    n1, n2, d = 1500, 400, 37
    x = (100.0 + 20.0 * rng.standard_normal((n1 + n2, d))).astype(np.float32)
    x[:n1] += 15.0  # the shards' means differ
    N = n1 + n2
    mu = x.astype(np.float64).mean(axis=0)
    ref = _cov_ref(x, mu)
    c = torch.from_numpy(mu)
    xt = torch.from_numpy(x).to(cuda)
    S = (de.sigma_hat_centered(xt[:n1], c) * (n1 / N) + de.sigma_hat_centered(xt[n1:], c) * (n2 / N))
    err = np.max(np.abs(S.cpu().numpy() - ref))
    bar = 1e-5 * np.max(np.abs(ref)) + 1e-12 * np.max(np.abs(ref))
    print(f"pooled from shards: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    own = (de.sigma_hat_centered(xt[:n1]) * (n1 / N) + de.sigma_hat_centered(xt[n1:]) * (n2 / N))
    assert np.max(np.abs(own.cpu().numpy() - ref)) > 100 * bar


# ---------------------------------------------------------------- fused centred transform
def _orthonormal(d, k, rng):
    """Orthonormal columns from a float64 QR, rounded to fp32; asymmetric content (a
    transposed or mirrored read of W would not go unnoticed)."""
    a = rng.standard_normal((d, k)) * np.linspace(1.0, 3.0, k) + np.linspace(0.0, 2.0, d)[:, None]
    return np.linalg.qr(a)[0].astype(np.float32)


class _Case:
    """Inputs on the device in strided, NaN-padded storage, and the float64 reference."""

    def __init__(self, n, d, k, cuda, mean_scale=5.0, offset=0.0, centred=True, seed=None):
        rng = np.random.default_rng(seed if seed is not None else 10000 * n + 10 * d + k)
        self.n, self.d, self.k, self.cuda = n, d, k, cuda
        self.orth = k <= d
        self.W = _orthonormal(d, k, rng) if self.orth else \
            (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
        mu = offset + mean_scale * rng.standard_normal(d)
        self.X = (mu + rng.standard_normal((n, d))).astype(np.float32)
        self.mean = self.X.astype(np.float64).mean(axis=0) if centred else None
        if centred and n == 1:
            self.mean = mu  # one row: its own mean would centre it to zero
        self.ldx, self.ldw, self.ldy = d + 4, d + 8, k + 1
        self.Xb = _padded(self.X, 4, cuda)
        self.Wb = _padded(np.ascontiguousarray(self.W.T), 8, cuda)  # column-major, ldw = d + 8
        self.mu_dev = None if self.mean is None else torch.from_numpy(self.mean).to(cuda)
        T = self.X.astype(np.float64) - (0.0 if self.mean is None else self.mean)
        W64 = self.W.astype(np.float64)
        self.T, self.W64 = T, W64
        self.Y_ref = T @ W64
        self.Y_bound = (d + 9) * U * (np.abs(T) @ np.abs(W64))
        self.en_ref = (T * T).sum(axis=1)
        self.res_ref = ((T - self.Y_ref @ W64.T) ** 2).sum(axis=1)

    def run(self, want=("Y", "resid", "energy"), ws=None, ws_bytes=None):
        L = _lib()
        n, d, k = self.n, self.d, self.k
        Y = torch.full((n, self.ldy), SENTINEL, dtype=torch.float32, device=self.cuda)
        res = torch.full((n,), SENTINEL, dtype=torch.float32, device=self.cuda)
        en = torch.full((n,), SENTINEL, dtype=torch.float32, device=self.cuda)
        if ws is None:
            ws_bytes = L.lib().deig_pca_transform_workspace(n, d, k)
            ws = _ws(ws_bytes, self.cuda)
        rc = L.lib().deig_pca_transform_f32(
            self.Xb.data_ptr(), n, d, self.ldx, None if self.mu_dev is None else self.mu_dev.data_ptr(),
            self.Wb.data_ptr(), k, self.ldw, Y.data_ptr() if "Y" in want else None, self.ldy,
            res.data_ptr() if "resid" in want else None, en.data_ptr() if "energy" in want else None,
            ws.data_ptr(), ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc, Y, res, en

    def ratios(self, Y, res, en):
        """Worst error over bound of each output (resid: orthonormal W only)."""
        y = Y[:, :self.k].cpu().numpy().astype(np.float64)
        safe = np.where(self.Y_bound > 0, self.Y_bound, 1.0)
        ry = float(np.max(np.where(self.Y_bound > 0, np.abs(y - self.Y_ref) / safe,
                                   np.abs(y - self.Y_ref))))
        e = en.cpu().numpy().astype(np.float64)
        eb = (self.d + 8) * U * self.en_ref
        re = float(np.max(np.abs(e - self.en_ref) / np.where(eb > 0, eb, 1.0)))
        rr = 0.0
        if self.orth:
            rb = (self.d + self.k + 8) * U * self.en_ref
            rr = float(np.max(np.abs(res.cpu().numpy().astype(np.float64) - self.res_ref)
                              / np.where(rb > 0, rb, 1.0)))
        return ry, re, rr


KS = [1, 3, 16, 17, 64, 200, 256]
DS = [4, 36, 260, 1028]
NS = [1, 63, 65, 129]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
def test_transform_edges(d, k, cuda):
    """Row-tile tails (n), chunk tails (d), every fragment count and k < kp (k); strided
    storage with NaN behind every row of X and column of W; the sentinel column of Y stays.
    k > d has no orthonormal W: Y and energy are checked there, resid only for its sign."""
    L = _lib()
    worst = [0.0, 0.0, 0.0]
    for n in NS:
        c = _Case(n, d, k, cuda)
        rc, Y, res, en = c.run()
        L.check(rc, "deig_pca_transform_f32")
        assert torch.all(Y[:, k] == SENTINEL), f"n={n}: wrote behind the k columns of Y"
        assert bool(torch.isfinite(Y[:, :k]).all()) and bool(torch.isfinite(res).all())
        assert bool((res >= 0).all())
        r = c.ratios(Y, res, en)
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1.0, f"n={n} d={d} k={k}: err / bound (Y, energy, resid) = {r}"
    print(f"pca_transform d={d} k={k}: worst err / bound Y {worst[0]:.4f} energy {worst[1]:.4f} "
          f"resid {worst[2]:.4f}")


@pytest.mark.parametrize("n,d,k", [(129, 260, 17), (65, 36, 3)])
def test_transform_subtracts_the_mean_before_the_product(n, d, k, cuda):
    """X = 1000 + N(0, 1): the kernel, like the float64 reference and an fp32 emulation of
    the subtract-first form, stays far inside the bounds; the post-hoc form
    X W - mean^T W in fp32 misses the Y bound by more than 10x."""
    c = _Case(n, d, k, cuda, mean_scale=0.0, offset=1000.0)
    # fp32 emulations on the CPU (sequential fp32 accumulation, the kernel's k order)
    t32 = (c.X.astype(np.float64) - c.mean).astype(np.float32)
    first = np.zeros((n, k), dtype=np.float32)
    post = np.zeros((n, k), dtype=np.float32)
    mw = np.zeros(k, dtype=np.float32)
    m32 = c.mean.astype(np.float32)
    for j in range(d):
        first += t32[:, j:j + 1] * c.W[j]
        post += c.X[:, j:j + 1] * c.W[j]
        mw += m32[j] * c.W[j]
    post -= mw
    r_first = float(np.max(np.abs(first - c.Y_ref) / c.Y_bound))
    r_post = float(np.max(np.abs(post - c.Y_ref) / c.Y_bound))
    assert r_first <= 0.1 and r_post > 10.0, (r_first, r_post)  # the data discriminates
    rc, Y, res, en = c.run()
    _lib().check(rc, "deig_pca_transform_f32")
    ry, re, rr = c.ratios(Y, res, en)
    print(f"mean 1000, n={n} d={d} k={k}: err / bound Y {ry:.4f} energy {re:.4f} resid {rr:.4f}; "
          f"emulations: subtract-first {r_first:.4f}, post-hoc {r_post:.1f}")
    assert max(ry, re, rr) <= 1.0
    assert ry <= 0.1, "the mean is not subtracted before the product"


@pytest.mark.parametrize("n,d,k", [(129, 260, 17), (65, 36, 3), (63, 1028, 64)])
def test_transform_outputs_alone_and_repeatable(n, d, k, cuda):
    c = _Case(n, d, k, cuda)
    rc, Y, res, en = c.run()
    _lib().check(rc, "deig_pca_transform_f32")
    rc2, Y2, res2, en2 = c.run()
    assert rc2 == 0 and torch.equal(Y, Y2) and torch.equal(res, res2) and torch.equal(en, en2)
    for want in (("Y",), ("resid",), ("energy",), ("Y", "energy")):
        rc1, Y1, res1, en1 = c.run(want)
        assert rc1 == 0, want
        assert torch.equal(Y1, Y) if "Y" in want else bool((Y1 == SENTINEL).all()), want
        assert torch.equal(res1, res) if "resid" in want else bool((res1 == SENTINEL).all()), want
        assert torch.equal(en1, en) if "energy" in want else bool((en1 == SENTINEL).all()), want


@pytest.mark.parametrize("n,d,k", [(129, 260, 17), (65, 36, 16), (1, 4, 1), (129, 1028, 256)])
def test_transform_without_a_mean_is_project(n, d, k, cuda):
    import distributed_eigenspaces_amd as de
    c = _Case(n, d, k, cuda, centred=False)
    rc, Y, res, en = c.run()
    _lib().check(rc, "deig_pca_transform_f32")
    bound = (d + 8) * U * (np.abs(c.T) @ np.abs(c.W64))  # the ``project`` bound
    y = Y[:, :k].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(y - c.Y_ref) <= bound)
    P = de.linalg.project(torch.from_numpy(c.X).to(cuda), torch.from_numpy(c.W).to(cuda))
    assert np.all(np.abs(y - P.cpu().numpy().astype(np.float64)) <= bound)
    # and the Python wrapper gives the kernel's bits
    Yw, rw, ew = de.pca_transform(torch.from_numpy(c.X).to(cuda), torch.from_numpy(c.W).to(cuda),
                                  residual=True, energy=True)
    assert torch.equal(Yw, Y[:, :k]) and torch.equal(rw, res) and torch.equal(ew, en)


def test_transform_wrapper_pads_columns(cuda):
    """d % 4 != 0 through the wrapper: zero columns, zero rows of W, zero mean entries."""
    import distributed_eigenspaces_amd as de
    rng = np.random.default_rng(3)
    n, d, k = 70, 37, 5
    W = _orthonormal(d, k, rng)
    X = (50.0 + rng.standard_normal((n, d))).astype(np.float32)
    mu = X.astype(np.float64).mean(axis=0)
    Y, res, en = de.pca_transform(torch.from_numpy(X).to(cuda), torch.from_numpy(W).to(cuda),
                                  torch.from_numpy(mu), residual=True, energy=True)
    T = X.astype(np.float64) - mu
    W64 = W.astype(np.float64)
    ref = T @ W64
    assert np.all(np.abs(Y.cpu().numpy() - ref) <= (d + 9) * U * (np.abs(T) @ np.abs(W64)))
    e_ref = (T * T).sum(axis=1)
    assert np.all(np.abs(en.cpu().numpy() - e_ref) <= (d + 8) * U * e_ref)
    r_ref = ((T - ref @ W64.T) ** 2).sum(axis=1)
    assert np.all(np.abs(res.cpu().numpy() - r_ref) <= (d + k + 8) * U * e_ref)
    # float64 samples: centred in float64 first
    Y64 = de.pca_transform(torch.from_numpy(X.astype(np.float64)).to(cuda),
                           torch.from_numpy(W).to(cuda), torch.from_numpy(mu))
    assert np.all(np.abs(Y64.cpu().numpy() - ref) <= (d + 9) * U * (np.abs(T) @ np.abs(W64)))


@pytest.mark.parametrize("n,d,k", [(129, 260, 17), (65, 1028, 256), (1, 4, 1)])
def test_transform_stays_in_workspace(n, d, k, cuda):
    L = _lib()
    c = _Case(n, d, k, cuda)
    nbytes = L.lib().deig_pca_transform_workspace(n, d, k)
    ws = _ws(nbytes, cuda, CANARY)
    rc, Y, res, en = c.run(ws=ws, ws_bytes=nbytes)
    L.check(rc, "deig_pca_transform_f32")
    assert int((ws[nbytes:] != FILL).sum()) == 0, "wrote past the workspace"
    assert max(c.ratios(Y, res, en)) <= 1.0


def test_transform_short_workspace_is_reported_and_outputs_untouched(cuda):
    L = _lib()
    c = _Case(65, 36, 3, cuda)
    nbytes = L.lib().deig_pca_transform_workspace(65, 36, 3)
    ws = _ws(nbytes, cuda)
    rc, Y, res, en = c.run(ws=ws, ws_bytes=nbytes - 1)
    assert rc == L.DEIG_EWORKSPACE and "workspace" in L.last_error()
    assert bool((Y == SENTINEL).all()) and bool((res == SENTINEL).all()) and bool((en == SENTINEL).all())
    assert bool((ws == FILL).all()), "GPU work before the workspace check"
