"""Centred PCA end to end (``pca.PCA``) against float64 numpy.

Data: n = 4096 samples in d = 256 with k = 4 planted directions of variance 61, 41, 26, 16
over unit noise and a mean of 200 in every coordinate (norm 3200: more than 50x the
largest spike, as a variance or as a standard deviation).  The float64 centred covariance
has lambda_k / lambda_{k+1} ~ 10 (asserted >= 4 below), so the 1e-4 projector bar of the
README resolves the top-k span; the uncentred second moment of the same data has the mean
direction on top, so the default estimator's basis is far from it.

Bars (README): ||P - P_ref||_F <= 1e-4, eigenvalues 1e-5 relative; the kernel bounds of
tests/test_gpu_pca_kernels.py for the scores and the reconstruction error."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

N, D, K = 4096, 256, 4
HELD = 100
P_TOL, EV_TOL = 1e-4, 1e-5
U = 2.0 ** -24


@functools.lru_cache(maxsize=1)
def _data():
    """(X float32 (N + HELD, D), float64 reference of the first N rows); shared, not written."""
    rng = np.random.default_rng(2024)
    Q = np.linalg.qr(rng.standard_normal((D, K)))[0]
    lam = np.array([60.0, 40.0, 25.0, 15.0])
    Z = rng.standard_normal((N + HELD, K)) * np.sqrt(lam)
    X = (200.0 + Z @ Q.T + rng.standard_normal((N + HELD, D))).astype(np.float32)
    x64 = X[:N].astype(np.float64)
    mu = x64.mean(axis=0)
    C = (x64 - mu).T @ (x64 - mu) / N
    w, V = np.linalg.eigh(C)
    assert w[-K] / w[-K - 1] >= 4.0, "the fixture's eigengap is too small for the bars"
    assert np.linalg.norm(mu) >= 50 * lam.max()
    ref = {"mu": mu, "w": w[::-1][:K].copy(), "V": V[:, ::-1][:, :K].copy(), "total": np.trace(C)}
    return X, ref


def _pdist(A, B):
    return ref_cpu.projector_distance(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))


@pytest.fixture(scope="module")
def fitted(cuda):
    from distributed_eigenspaces_amd import PCA
    X, _ = _data()
    return PCA(K).fit(torch.from_numpy(X[:N]).to(cuda))


def test_the_uncentred_fit_is_somewhere_else(cuda):
    """The data discriminates: the existing (uncentred) estimator's basis is far from the
    centred one - its top vector is the mean direction."""
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    X, ref = _data()
    r = DistributedEigenspaceEstimator(K).fit(torch.from_numpy(X[:N]).to(cuda))
    V = r.V.cpu().numpy()
    assert _pdist(V, ref["V"]) > 0.5
    ones = np.ones(D) / np.sqrt(D)
    # (the server's columns are fixed only as a span: a projector average of one basis)
    assert np.linalg.norm(V.T @ ones) > 0.999


def test_one_worker_matches_float64_eigh(fitted):
    _, ref = _data()
    p = fitted
    assert p.n_samples_ == N
    assert p.mean_.dtype == torch.float64
    np.testing.assert_allclose(p.mean_.cpu().numpy(), ref["mu"], rtol=1e-12)
    comp = p.components_.cpu().numpy()
    assert comp.shape == (K, D)
    dist = _pdist(comp.T, ref["V"])
    ev = p.explained_variance_.cpu().numpy()
    ev_ref = ref["w"] * N / (N - 1)  # sklearn's divisor
    ratio = p.explained_variance_ratio_.cpu().numpy()
    print(f"PCA one worker: ||P - P_ref||_F = {dist:.2e}, explained variance rel err "
          f"{np.max(np.abs(ev - ev_ref) / ev_ref):.2e}")
    assert dist <= P_TOL
    assert np.all(np.diff(ev) < 0), "components are not in descending variance"
    np.testing.assert_allclose(ev, ev_ref, rtol=EV_TOL)
    np.testing.assert_allclose(ratio, ref["w"] / ref["total"], atol=1e-5, rtol=0)
    # the components are the principal axes themselves, not only their span
    assert np.all(np.abs(np.sum(comp.T * ref["V"], axis=0)) >= 1 - 1e-6)
    np.testing.assert_allclose(comp @ comp.T, np.eye(K), atol=1e-5)


def test_four_workers_match_the_float64_emulation(cuda):
    """workers_per_rank = 4 == the same algorithm in float64 numpy: shards centred about
    the POOLED mean, per-shard eigh, projector average, eigh."""
    from distributed_eigenspaces_amd import PCA
    X, ref = _data()
    p = PCA(K, workers_per_rank=4).fit(torch.from_numpy(X[:N]).to(cuda))
    x64 = X[:N].astype(np.float64)
    mu = x64.mean(axis=0)
    Pbar = np.zeros((D, D))
    for lo, hi in ref_cpu.split_batches(N, 4):
        t = x64[lo:hi] - mu
        V = np.linalg.eigh(t.T @ t / (hi - lo))[1][:, -K:]
        Pbar += V @ V.T / 4
    Vs = np.linalg.eigh(Pbar)[1][:, -K:]
    dist = _pdist(p.components_.cpu().numpy().T, Vs)
    print(f"PCA four workers: ||P - P_emulated||_F = {dist:.2e}")
    assert dist <= P_TOL
    np.testing.assert_allclose(p.mean_.cpu().numpy(), mu, rtol=1e-12)
    assert p.n_samples_ == N
    assert np.all(np.diff(p.explained_variance_.cpu().numpy()) < 0)


def test_model_use_on_held_out_rows(fitted, cuda):
    X, _ = _data()
    p = fitted
    H = X[N:]
    Ht = torch.from_numpy(H).to(cuda)
    Y = p.transform(Ht)
    res = p.reconstruction_error(Ht)
    assert Y.shape == (HELD, K) and res.shape == (HELD,)
    W = p.components_.cpu().numpy().astype(np.float64).T
    T = H.astype(np.float64) - p.mean_.cpu().numpy()
    y_ref = T @ W
    assert np.all(np.abs(Y.cpu().numpy() - y_ref) <= (D + 9) * U * (np.abs(T) @ np.abs(W)))
    energy = (T * T).sum(axis=1)
    r_ref = ((T - y_ref @ W.T) ** 2).sum(axis=1)
    assert np.all(np.abs(res.cpu().numpy() - r_ref) <= (D + K + 8) * U * energy)
    # inverse_transform(transform(X)) is X minus the residual vector
    back = p.inverse_transform(Y).cpu().numpy().astype(np.float64)
    want = H.astype(np.float64) - (T - y_ref @ W.T)
    assert np.linalg.norm(back - want) <= 1e-5 * np.linalg.norm(want)


def test_float64_samples(cuda):
    from distributed_eigenspaces_amd import PCA
    X, ref = _data()
    p = PCA(K).fit(torch.from_numpy(X[:N].astype(np.float64)).to(cuda))
    assert _pdist(p.components_.cpu().numpy().T, ref["V"]) <= P_TOL
    np.testing.assert_allclose(p.explained_variance_.cpu().numpy(), ref["w"] * N / (N - 1), rtol=EV_TOL)


def test_uint8_samples_are_rejected(cuda):
    from distributed_eigenspaces_amd import PCA
    with pytest.raises(TypeError, match="uint8"):
        PCA(K).fit(torch.zeros((64, 16), dtype=torch.uint8, device=cuda))


def test_matches_sklearn(fitted, cuda):
    skd = pytest.importorskip("sklearn.decomposition")
    X, _ = _data()
    sk = skd.PCA(n_components=K, svd_solver="full").fit(X[:N].astype(np.float64))
    p = fitted
    assert _pdist(p.components_.cpu().numpy().T, sk.components_.T) <= P_TOL
    np.testing.assert_allclose(p.explained_variance_.cpu().numpy(), sk.explained_variance_, rtol=EV_TOL)
    H = X[N:]
    Y = p.transform(torch.from_numpy(H).to(cuda)).cpu().numpy()
    Ys = sk.transform(H.astype(np.float64))
    signs = np.sign(np.sum(p.components_.cpu().numpy() * sk.components_, axis=1))
    np.testing.assert_allclose(Y * signs, Ys, atol=1e-3 * np.abs(Ys).max())


# ---------------------------------------------------------------- gloo world 2, GPU workers
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_rank(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributed_eigenspaces_amd import PCA
    X, _ = _data()
    half = N // world
    p = PCA(K).fit(torch.from_numpy(X[rank * half:(rank + 1) * half]).cuda())
    torch.save({"mean": p.mean_.cpu(), "components": p.components_.cpu(),
                "ev": p.explained_variance_.cpu(), "n": p.n_samples_},
               os.path.join(out, f"pca{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_with_gpu_workers(tmp_path, cuda):
    """Two ranks (sharing cuda:0, talking gloo) end with the same mean_ and components_,
    those of the single-process fit with two workers on the concatenated rows."""
    from distributed_eigenspaces_amd import PCA
    mp.spawn(_run_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(os.path.join(tmp_path, "pca0.pt"), weights_only=True)
    r1 = torch.load(os.path.join(tmp_path, "pca1.pt"), weights_only=True)
    assert r0["n"] == r1["n"] == N
    assert torch.equal(r0["mean"], r1["mean"]) and torch.equal(r0["components"], r1["components"])
    assert torch.equal(r0["ev"], r1["ev"])
    X, _ = _data()
    one = PCA(K, workers_per_rank=2).fit(torch.from_numpy(X[:N]).to(cuda))
    # the pooled mean: column sums added in another order (last-ulp differences)
    np.testing.assert_allclose(r0["mean"].numpy(), one.mean_.cpu().numpy(), rtol=1e-14)
    c0, c1 = r0["components"].numpy(), one.components_.cpu().numpy()
    assert _pdist(c0.T, c1.T) <= 1e-5
    assert np.all(np.abs(np.sum(c0 * c1, axis=1)) >= 1 - 1e-6)
    np.testing.assert_allclose(r0["ev"].numpy(), one.explained_variance_.cpu().numpy(), rtol=1e-6)
