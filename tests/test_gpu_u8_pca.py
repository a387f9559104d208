"""Centred PCA of uint8 samples end to end (``PCA(k, u8_mode=...)``) against float64 numpy.

Data: a planted spiked model on the 0..255 grid, as tests/test_gpu_cifar.py builds it
(clip(round(128 + 20 (G + H sqrt(theta) U^T))), theta 8 -> 4): N = 4096 rows (+ 1000 held
out), d = 64 raw bytes, or 8 x 8 x 3 pixels whose grey values are the 64 features; k = 4.
The project's bars apply to the axes only if the spectrum separates them: asserted on the
CPU, before anything runs on the GPU, that in float64 ``eigh`` of the exact centred
covariance the gap below the k-th eigenvalue and the gaps between the top k are each >= 5 %
of the k-th / the lower eigenvalue.

Bars (README): ||P - P_ref||_F <= 1e-4, explained variance 1e-5 relative (divisor N - 1),
mean 1e-13 relative; the kernel bounds of tests/test_gpu_u8_pca_kernels.py for the scores and
the reconstruction error of held-out rows."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

N, HELD, D, K = 4096, 1000, 64, 4
P_TOL, EV_TOL, MEAN_TOL = 1e-4, 1e-5, 1e-13
U = 2.0 ** -24
MODES = ["raw", "gray"]


def _spiked_bytes(n, d, k, seed, scale=20.0, channels=0):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((d, k)))[0]
    sig = (rng.standard_normal((n, k)) * np.sqrt(np.linspace(8.0, 4.0, k))) @ Q.T
    if channels:
        out = np.empty((n, d, channels), dtype=np.uint8)
        for c in range(channels):
            x = rng.standard_normal((n, d)) + sig
            out[:, :, c] = np.clip(np.rint(128.0 + scale * x), 0, 255)
        return out
    return np.clip(np.rint(128.0 + scale * (rng.standard_normal((n, d)) + sig)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def _data(mode):
    """(bytes as the fit takes them, features v float64 (N + HELD, D), float64 reference of the
    first N rows); shared, not written.  The condition on the spectrum is asserted here."""
    if mode == "raw":
        x = _spiked_bytes(N + HELD, D, K, seed=11)
        v = x.astype(np.float64)
    else:
        x = _spiked_bytes(N + HELD, D, K, seed=12, channels=3).reshape(N + HELD, 8, 8, 3)
        v = x.astype(np.float64).sum(axis=3).reshape(N + HELD, D) / 3.0
    mu = v[:N].mean(axis=0)
    t = v[:N] - mu
    C = t.T @ t / N
    w, V = np.linalg.eigh(C)
    top = w[::-1][:K + 1]
    assert top[K - 1] - top[K] >= 0.05 * top[K - 1], "no gap below the k-th eigenvalue"
    assert np.all(top[:K - 1] - top[1:K] >= 0.05 * top[1:K]), "the top k are not separated"
    ref = {"mu": mu, "w": top[:K].copy(), "V": V[:, ::-1][:, :K].copy(), "total": np.trace(C)}
    return x, v, ref


def _pdist(A, B):
    return ref_cpu.projector_distance(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))


@functools.lru_cache(maxsize=2)
def _fit(mode):
    from distributed_eigenspaces_amd import PCA
    x, _, _ = _data(mode)
    return PCA(K, u8_mode=mode).fit(torch.from_numpy(x[:N]).to("cuda:0"))


@pytest.mark.parametrize("mode", MODES)
def test_matches_float64_eigh(mode, cuda):
    _, _, ref = _data(mode)
    p = _fit(mode)
    assert p.n_samples_ == N
    assert p.mean_.dtype == torch.float64 and p.mean_.shape == (D,)
    np.testing.assert_allclose(p.mean_.cpu().numpy(), ref["mu"], rtol=MEAN_TOL)
    comp = p.components_.cpu().numpy()
    assert comp.shape == (K, D)
    dist = _pdist(comp.T, ref["V"])
    ev = p.explained_variance_.cpu().numpy()
    ev_ref = ref["w"] * N / (N - 1)  # sklearn's divisor
    print(f"u8 PCA {mode}: ||P - P_ref||_F = {dist:.2e}, explained variance rel err "
          f"{np.max(np.abs(ev - ev_ref) / ev_ref):.2e}")
    assert dist <= P_TOL
    assert np.all(np.diff(ev) < 0), "components are not in descending variance"
    np.testing.assert_allclose(ev, ev_ref, rtol=EV_TOL)
    np.testing.assert_allclose(p.explained_variance_ratio_.cpu().numpy(), ref["w"] / ref["total"],
                               atol=1e-5, rtol=0)
    # the principal axes themselves, not only their span
    assert np.all(np.abs(np.sum(comp.T * ref["V"], axis=0)) >= 1 - 1e-6)


@pytest.mark.parametrize("mode", MODES)
def test_agrees_with_the_float64_path(mode, cuda):
    from distributed_eigenspaces_amd import PCA
    _, v, _ = _data(mode)
    p = _fit(mode)
    f = PCA(K).fit(torch.from_numpy(v[:N]).to(cuda))
    assert _pdist(p.components_.cpu().numpy().T, f.components_.cpu().numpy().T) <= P_TOL
    np.testing.assert_allclose(p.explained_variance_.cpu().numpy(),
                               f.explained_variance_.cpu().numpy(), rtol=EV_TOL)
    np.testing.assert_allclose(p.mean_.cpu().numpy(), f.mean_.cpu().numpy(), rtol=MEAN_TOL)


@pytest.mark.parametrize("mode", MODES)
def test_four_workers_match_the_float64_emulation(mode, cuda):
    """workers_per_rank = 4 == the same algorithm in float64 numpy: shards centred about the
    POOLED mean, per-shard eigh, projector average, eigh."""
    from distributed_eigenspaces_amd import PCA
    x, v, _ = _data(mode)
    p = PCA(K, workers_per_rank=4, u8_mode=mode).fit(torch.from_numpy(x[:N]).to(cuda))
    mu = v[:N].mean(axis=0)
    Pbar = np.zeros((D, D))
    for lo, hi in ref_cpu.split_batches(N, 4):
        t = v[lo:hi] - mu
        V = np.linalg.eigh(t.T @ t / (hi - lo))[1][:, -K:]
        Pbar += V @ V.T / 4
    Vs = np.linalg.eigh(Pbar)[1][:, -K:]
    dist = _pdist(p.components_.cpu().numpy().T, Vs)
    print(f"u8 PCA {mode}, four workers: ||P - P_emulated||_F = {dist:.2e}")
    assert dist <= P_TOL
    np.testing.assert_allclose(p.mean_.cpu().numpy(), mu, rtol=MEAN_TOL)
    assert p.n_samples_ == N
    assert np.all(np.diff(p.explained_variance_.cpu().numpy()) < 0)


@pytest.mark.parametrize("mode", MODES)
def test_model_use_on_held_out_rows(mode, cuda):
    x, v, _ = _data(mode)
    p = _fit(mode)
    Ht = torch.from_numpy(x[N:]).to(cuda)
    Y = p.transform(Ht)
    res = p.reconstruction_error(Ht)
    assert Y.shape == (HELD, K) and res.shape == (HELD,)
    W = p.components_.cpu().numpy().astype(np.float64).T
    T = v[N:] - p.mean_.cpu().numpy()
    y_ref = T @ W
    assert np.all(np.abs(Y.cpu().numpy() - y_ref) <= (D + 9) * U * (np.abs(T) @ np.abs(W)))
    energy = (T * T).sum(axis=1)
    r_ref = ((T - y_ref @ W.T) ** 2).sum(axis=1)
    assert np.all(np.abs(res.cpu().numpy() - r_ref) <= (D + K + 8) * U * energy)
    # inverse_transform is unchanged: float rows in v-space
    back = p.inverse_transform(Y).cpu().numpy().astype(np.float64)
    want = v[N:] - (T - y_ref @ W.T)
    assert np.linalg.norm(back - want) <= 1e-5 * np.linalg.norm(want)


def test_the_estimator_is_what_the_fit_runs(cuda):
    """DistributedEigenspaceEstimator(center=True, u8_mode="raw") on the same bytes: the mean
    of the PCA fit bit for bit, and the span of its components."""
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    x, _, ref = _data("raw")
    p = _fit("raw")
    r = DistributedEigenspaceEstimator(K, center=True, u8_mode="raw").fit(torch.from_numpy(x[:N]).to(cuda))
    assert torch.equal(r.mean, p.mean_)
    V = r.V.cpu().numpy()
    assert _pdist(V, p.components_.cpu().numpy().T) <= 1e-5
    assert _pdist(V, ref["V"]) <= P_TOL
    # and without the keyword the estimator widens uint8 as before: the same matrix, float path
    r0 = DistributedEigenspaceEstimator(K, center=True).fit(torch.from_numpy(x[:N]).to(cuda))
    assert _pdist(r0.V.cpu().numpy(), ref["V"]) <= P_TOL
    with pytest.raises(ValueError, match="center=True"):
        DistributedEigenspaceEstimator(K, u8_mode="raw")


def test_uint8_without_the_keyword_is_still_rejected(cuda):
    from distributed_eigenspaces_amd import PCA
    x, _, _ = _data("raw")
    with pytest.raises(TypeError, match="uint8.*u8_mode"):
        PCA(K).fit(torch.from_numpy(x[:64]).to(cuda))
    with pytest.raises(ValueError, match="u8_mode"):
        PCA(K, u8_mode="grey")
