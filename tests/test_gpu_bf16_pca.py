"""bf16 samples through the centred stack without widening them: DEIG_BF16 in the column
passes (bit-identical to the float32 copy), the fused bf16 transform
(deig_pca_transform_bf16) at the bounds tests/test_gpu_pca_kernels.py applies to the float
kernel, and the estimator and ``PCA`` on bfloat16 tensors against float64 of the same bf16
values.

Transform bounds, with u = 2^-24 and t = x - mean in float64 (x the bf16 value):
  |Y - ref| <= (d + 9) u (|t| |W|),  |energy - ref| <= (d + 8) u ref,
  |resid - ||t - W W^T t||^2| <= (d + k + 8) u energy.
Estimator and PCA bars (README): ||P - P_ref||_F <= 1e-4, eigenvalues 1e-5 relative."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 777.0
P_TOL, EV_TOL = 1e-4, 1e-5


def _lib():
    from distributed_eigenspaces_amd import _lib as L
    return L


def _bf16(a):
    """float array -> (torch.bfloat16 CPU tensor, its float64 numpy values)."""
    t = torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t, t.double().numpy()


# ---------------------------------------------------------------- column passes: same bits
@pytest.mark.parametrize("n,d", [(1000, 264), (5000, 1032)])
def test_column_passes_give_the_bits_of_the_float32_copy(n, d, cuda):
    import distributed_eigenspaces_amd as de
    rng = np.random.default_rng(n + d)
    xb, x64 = _bf16(10.0 + 3.0 * rng.standard_normal((n, d)))
    xb = xb.to(cuda)
    xf = xb.float()
    s_b, s_f = de.column_sums(xb), de.column_sums(xf)
    assert s_b.dtype == torch.float64 and torch.equal(s_b, s_f)
    np.testing.assert_allclose(s_b.cpu().numpy(), x64.sum(axis=0), rtol=1e-12)
    # a strided bf16 view (row stride d + 8, NaN behind the rows) reads the same values
    buf = torch.full((n, d + 8), float("nan"), dtype=torch.bfloat16, device=cuda)
    buf[:, :d] = xb
    assert torch.equal(de.column_sums(buf[:, :d]), s_f)
    shifted = torch.from_numpy(x64.mean(axis=0) + 0.25).to(cuda)
    for c in (None, torch.zeros(d, dtype=torch.float64, device=cuda), shifted):
        Sb, mb = de.sigma_hat_centered(xb, center=c, return_mean=True)
        Sf, mf = de.sigma_hat_centered(xf, center=c, return_mean=True)
        assert torch.equal(Sb, Sf) and torch.equal(mb, mf)
        assert torch.equal(de.sigma_hat_centered(xb, center=c, dtype=torch.float32),
                           de.sigma_hat_centered(xf, center=c, dtype=torch.float32))
    Sb = de.sigma_hat(xb, shift=True)
    assert Sb.dtype == torch.float64 and torch.equal(Sb, de.sigma_hat(xf, shift=True))
    assert torch.equal(de.sigma_hat(buf[:, :d], shift=True), Sb)
    ref = x64.T @ x64 / n
    assert np.abs(Sb.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---------------------------------------------------------------- fused bf16 transform
def _orthonormal(d, k, rng):
    a = rng.standard_normal((d, k)) * np.linspace(1.0, 3.0, k) + np.linspace(0.0, 2.0, d)[:, None]
    return np.linalg.qr(a)[0].astype(np.float32)


class _Case:
    """bf16 inputs on the device in strided, NaN-padded storage and the float64 reference."""

    def __init__(self, n, d, k, cuda, centred):
        rng = np.random.default_rng(10000 * n + 10 * d + k + (1 if centred else 0))
        self.n, self.d, self.k, self.cuda = n, d, k, cuda
        self.orth = k <= d
        self.W = _orthonormal(d, k, rng) if self.orth else \
            (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
        mu = 5.0 * rng.standard_normal(d)
        xb, self.X64 = _bf16(mu + rng.standard_normal((n, d)))
        self.mean = None
        if centred:
            self.mean = self.X64.mean(axis=0) if n > 1 else mu
        self.ldx, self.ldw, self.ldy = d + 8, d + 8, k + 1
        self.Xb = torch.full((n, self.ldx), float("nan"), dtype=torch.bfloat16, device=cuda)
        self.Xb[:, :d] = xb.to(cuda)
        self.Wb = torch.full((k, self.ldw), float("nan"), dtype=torch.float32, device=cuda)
        self.Wb[:, :d] = torch.from_numpy(np.ascontiguousarray(self.W.T)).to(cuda)  # column-major
        self.mu_dev = None if self.mean is None else torch.from_numpy(self.mean).to(cuda)
        T = self.X64 - (0.0 if self.mean is None else self.mean)
        W64 = self.W.astype(np.float64)
        self.T, self.W64 = T, W64
        self.Y_ref = T @ W64
        self.Y_bound = (d + 9) * U * (np.abs(T) @ np.abs(W64))
        self.en_ref = (T * T).sum(axis=1)
        self.res_ref = ((T - self.Y_ref @ W64.T) ** 2).sum(axis=1)

    def run(self, want=("Y", "resid", "energy")):
        L = _lib()
        n, d, k = self.n, self.d, self.k
        Y = torch.full((n, self.ldy), SENTINEL, dtype=torch.float32, device=self.cuda)
        res = torch.full((n,), SENTINEL, dtype=torch.float32, device=self.cuda)
        en = torch.full((n,), SENTINEL, dtype=torch.float32, device=self.cuda)
        nbytes = L.lib().deig_pca_transform_bf16_workspace(n, d, k)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=self.cuda)  # NaN-poisoned
        rc = L.lib().deig_pca_transform_bf16(
            self.Xb.data_ptr(), n, d, self.ldx, None if self.mu_dev is None else self.mu_dev.data_ptr(),
            self.Wb.data_ptr(), k, self.ldw, Y.data_ptr() if "Y" in want else None, self.ldy,
            res.data_ptr() if "resid" in want else None, en.data_ptr() if "energy" in want else None,
            ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        L.check(rc, "deig_pca_transform_bf16")
        torch.cuda.synchronize()
        return Y, res, en

    def ratios(self, Y, res, en):
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


@pytest.mark.parametrize("k", [1, 16, 17, 64, 256])
@pytest.mark.parametrize("d", [8, 72, 136, 1032])
def test_transform_edges(d, k, cuda):
    """A short tail (d = 8), a partial super-chunk (72), several (136, 1032); row-tile tails;
    every fragment count and k < kp; with and without a mean; NaN behind every row of X and
    column of W; the sentinel column of Y stays.  k > d has no orthonormal W: resid is then
    checked only for its sign."""
    worst = [0.0, 0.0, 0.0]
    for n in (1, 63, 65, 1000):
        for centred in (True, False):
            c = _Case(n, d, k, cuda, centred)
            Y, res, en = c.run()
            assert torch.all(Y[:, k] == SENTINEL), f"n={n}: wrote behind the k columns of Y"
            assert bool(torch.isfinite(Y[:, :k]).all()) and bool(torch.isfinite(res).all())
            assert bool((res >= 0).all())
            r = c.ratios(Y, res, en)
            worst = [max(a, b) for a, b in zip(worst, r)]
            assert max(r) <= 1.0, f"n={n} d={d} k={k} centred={centred}: err / bound = {r}"
    print(f"pca_transform_bf16 d={d} k={k}: worst err / bound Y {worst[0]:.4f} energy "
          f"{worst[1]:.4f} resid {worst[2]:.4f}")


@pytest.mark.parametrize("n,d,k", [(65, 72, 3), (1000, 136, 17), (63, 1032, 64)])
def test_transform_outputs_alone_repeatable_and_wrapped(n, d, k, cuda):
    import distributed_eigenspaces_amd as de
    c = _Case(n, d, k, cuda, True)
    Y, res, en = c.run()
    Y2, res2, en2 = c.run()
    assert torch.equal(Y, Y2) and torch.equal(res, res2) and torch.equal(en, en2)
    for want in (("Y",), ("resid",), ("energy",)):
        Y1, res1, en1 = c.run(want)
        assert torch.equal(Y1, Y) if "Y" in want else bool((Y1 == SENTINEL).all()), want
        assert torch.equal(res1, res) if "resid" in want else bool((res1 == SENTINEL).all()), want
        assert torch.equal(en1, en) if "energy" in want else bool((en1 == SENTINEL).all()), want
    # the Python wrapper on the strided view gives the kernel's bits
    Yw, rw, ew = de.pca_transform(c.Xb[:, :d], torch.from_numpy(c.W).to(cuda), c.mu_dev,
                                  residual=True, energy=True)
    assert torch.equal(Yw, Y[:, :k]) and torch.equal(rw, res) and torch.equal(ew, en)
    # without a mean the staged values are the exact widening: the float kernel's inputs
    c0 = _Case(n, d, k, cuda, False)
    Y0, _, _ = c0.run()
    Yf = de.pca_transform(c0.Xb[:, :d].float(), torch.from_numpy(c0.W).to(cuda))
    assert np.all(np.abs(Y0[:, :k].cpu().numpy().astype(np.float64)
                         - Yf.cpu().numpy().astype(np.float64)) <= 2 * c0.Y_bound)


def test_transform_wrapper_pads_columns(cuda):
    """d % 8 != 0 through the wrapper: a zero-padded bf16 copy, zero rows of W."""
    import distributed_eigenspaces_amd as de
    rng = np.random.default_rng(3)
    n, d, k = 70, 37, 5
    W = _orthonormal(d, k, rng)
    xb, x64 = _bf16(20.0 + rng.standard_normal((n, d)))
    mu = x64.mean(axis=0)
    Y, en = de.pca_transform(xb.to(cuda), torch.from_numpy(W).to(cuda), torch.from_numpy(mu),
                             energy=True)
    T = x64 - mu
    W64 = W.astype(np.float64)
    assert np.all(np.abs(Y.cpu().numpy() - T @ W64) <= (d + 9) * U * (np.abs(T) @ np.abs(W64)))
    e_ref = (T * T).sum(axis=1)
    assert np.all(np.abs(en.cpu().numpy() - e_ref) <= (d + 8) * U * e_ref)
    S = de.sigma_hat(xb.to(cuda))  # the covariance wrapper pads the same way
    ref = x64.T @ x64 / n
    assert S.shape == (d, d) and np.abs(S.cpu().numpy() - ref).max() <= 2e-6 * np.abs(ref).max()


# ---------------------------------------------------------------- estimator
EN, ED, EK, EW = 8192, 512, 8, 4


@functools.lru_cache(maxsize=2)
def _spiked(mean):
    """Planted spiked data (8 directions of variance 40 .. 12 over unit noise, every coordinate
    shifted by ``mean``) rounded to bf16: (bf16 CPU tensor, its float64 values)."""
    rng = np.random.default_rng(99)
    Q = np.linalg.qr(rng.standard_normal((ED, EK)))[0]
    lam = np.linspace(40.0, 12.0, EK)
    Z = rng.standard_normal((EN, EK)) * np.sqrt(lam)
    return _bf16(mean + Z @ Q.T + rng.standard_normal((EN, ED)))


def _emulate(x64, center):
    """The estimator's algorithm in float64: per-shard covariance (about the pooled mean when
    centred), eigh, projector average, eigh."""
    mu = x64.mean(axis=0) if center else np.zeros(x64.shape[1])
    Pbar = np.zeros((ED, ED))
    wev = []
    for lo, hi in ref_cpu.split_batches(EN, EW):
        t = x64[lo:hi] - mu
        w, V = np.linalg.eigh(t.T @ t / (hi - lo))
        wev.append(w[-EK:])
        Pbar += V[:, -EK:] @ V[:, -EK:].T / EW
    w, V = np.linalg.eigh(Pbar)
    return V[:, -EK:], w[-EK:], wev, mu


@pytest.mark.parametrize("center", [False, True])
def test_estimator_on_bf16_samples(center, cuda):
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    xb, x64 = _spiked(0.5 if center else 0.0)  # the uncentred fit keeps its k planted directions
    r = DistributedEigenspaceEstimator(k=EK, workers_per_rank=EW, center=center).fit(xb.to(cuda))
    Vr, wr, wev, mu = _emulate(x64, center)
    dist = ref_cpu.projector_distance(r.V.cpu().numpy().astype(np.float64), Vr)
    ev = r.evals.cpu().numpy().astype(np.float64)
    rel = float(np.max(np.abs(ev - wr) / np.abs(wr)))
    wrel = max(float(np.max(np.abs(g.cpu().numpy().astype(np.float64) - w) / w))
               for g, w in zip(r.worker_evals, wev))
    print(f"bf16 estimator center={center}: ||P - P_ref||_F = {dist:.2e}, server evals rel "
          f"{rel:.2e}, worker evals rel {wrel:.2e}")
    assert dist <= P_TOL
    assert rel <= EV_TOL and wrel <= EV_TOL
    if center:
        np.testing.assert_allclose(r.mean.cpu().numpy(), mu, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------- PCA
PN, PD, PK, HELD = 4096, 256, 4, 100


@functools.lru_cache(maxsize=1)
def _pca_data():
    rng = np.random.default_rng(2024)
    Q = np.linalg.qr(rng.standard_normal((PD, PK)))[0]
    lam = np.array([60.0, 40.0, 25.0, 15.0])
    Z = rng.standard_normal((PN + HELD, PK)) * np.sqrt(lam)
    xb, x64 = _bf16(20.0 + Z @ Q.T + rng.standard_normal((PN + HELD, PD)))
    fit = x64[:PN]
    mu = fit.mean(axis=0)
    C = (fit - mu).T @ (fit - mu) / PN
    w, V = np.linalg.eigh(C)
    assert w[-PK] / w[-PK - 1] >= 4.0, "the fixture's eigengap is too small for the bars"
    return xb, x64, {"mu": mu, "w": w[::-1][:PK].copy(), "V": V[:, ::-1][:, :PK].copy()}


def test_pca_on_bf16_samples(cuda):
    from distributed_eigenspaces_amd import PCA
    xb, x64, ref = _pca_data()
    xg = xb.to(cuda)
    p = PCA(PK).fit(xg[:PN])
    assert p.n_samples_ == PN
    assert p.mean_.dtype == torch.float64 and p.components_.dtype == torch.float32
    np.testing.assert_allclose(p.mean_.cpu().numpy(), ref["mu"], rtol=1e-12)
    comp = p.components_.cpu().numpy()
    assert comp.shape == (PK, PD)
    dist = ref_cpu.projector_distance(comp.T.astype(np.float64), ref["V"])
    ev = p.explained_variance_.cpu().numpy()
    ev_ref = ref["w"] * PN / (PN - 1)
    print(f"bf16 PCA: ||P - P_ref||_F = {dist:.2e}, explained variance rel err "
          f"{np.max(np.abs(ev - ev_ref) / ev_ref):.2e}")
    assert dist <= P_TOL
    np.testing.assert_allclose(ev, ev_ref, rtol=EV_TOL)
    assert np.all(np.abs(np.sum(comp.T * ref["V"], axis=0)) >= 1 - 1e-6)
    # model use on held-out bf16 rows: no TypeError, the kernel bounds against float64, and
    # agreement with the float path on the widened rows
    H = xg[PN:]
    Y = p.transform(H)
    res = p.reconstruction_error(H)
    assert Y.shape == (HELD, PK) and res.shape == (HELD,)
    W = comp.astype(np.float64).T
    T = x64[PN:] - p.mean_.cpu().numpy()
    y_ref = T @ W
    yb = (PD + 9) * U * (np.abs(T) @ np.abs(W))
    assert np.all(np.abs(Y.cpu().numpy() - y_ref) <= yb)
    energy = (T * T).sum(axis=1)
    r_ref = ((T - y_ref @ W.T) ** 2).sum(axis=1)
    rb = (PD + PK + 8) * U * energy
    assert np.all(np.abs(res.cpu().numpy() - r_ref) <= rb)
    Yf, resf = p.transform(H.float()), p.reconstruction_error(H.float())
    assert np.all(np.abs(Y.cpu().numpy().astype(np.float64) - Yf.cpu().numpy()) <= 2 * yb)
    assert np.all(np.abs(res.cpu().numpy().astype(np.float64) - resf.cpu().numpy()) <= 2 * rb)
