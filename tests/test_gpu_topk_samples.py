"""The covariance-free worker solve (linalg.topk_samples, deig_topk_samples) and the routes
built on it: DistributedEigenspaceEstimator(covariance="free") and PCA(covariance="free").

The bars are the project's (test_gpu_pipeline.py): ||P - P_ref||_F <= 1e-4 and eigenvalues to
1e-5 relative, always against float64 references - the reference run's golden outputs, or
NumPy on the staged matrix Xc = fl32((double)x - c) - never against the explicit GPU route."""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.conftest import load_golden
from tests.golden_data import spiked_int_data

pytestmark = pytest.mark.gpu
P_TOL, EV_TOL = 1e-4, 1e-5


def _staged(x: torch.Tensor, c):
    """Xc as float64 NumPy: what the kernels stage."""
    x64 = x.cpu().to(torch.float64)
    if c is None:
        return x64.numpy()
    return (x64 - torch.as_tensor(c, dtype=torch.float64)).to(torch.float32).to(torch.float64).numpy()


def _check(r, V_ref, w_ref):
    assert r.converged
    V = r.V.cpu().numpy()
    dist = ref_cpu.projector_distance(V, V_ref)
    ev = r.evals.cpu().numpy()
    rel = np.max(np.abs(ev - w_ref) / np.abs(w_ref))
    print(f"projector distance {dist:.3e}, eigenvalue error {rel:.3e}, sweeps {r.sweeps}")
    assert dist <= P_TOL
    np.testing.assert_allclose(ev, w_ref, rtol=EV_TOL)
    assert r.V.stride(0) == 1  # column-major


@pytest.mark.parametrize("name", ["spiked_d256_k10_m8", "spiked_d64_k4_m8"])
def test_golden_workers(name, cuda):
    """Every shard's topk_samples against the reference run's worker outputs (zero-mean data)."""
    import distributed_eigenspaces_amd as de
    g = load_golden(name)
    k = int(g["k"])
    X = torch.from_numpy(g["X"].astype(np.float32)).to(cuda)
    for i, (lo, hi) in enumerate(np.asarray(g["ranges"]).reshape(-1, 2)):
        r = de.topk_samples(X[int(lo):int(hi)], k)
        _check(r, g["worker_V"][i], np.sort(np.asarray(g["worker_evals"][i], dtype=np.float64)))


@functools.lru_cache(maxsize=None)
def _centred_inputs():
    Xq, _ = spiked_int_data(1500, 132, 4, seed=11)
    assert Xq.min() >= -128 and Xq.max() <= 127  # none clip
    return Xq


def _forms(Xq, dev):
    return {"u8": torch.from_numpy((Xq + 128).astype(np.uint8)).to(dev),
            "f32": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev),
            "bf16": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev).to(torch.bfloat16)}


@functools.lru_cache(maxsize=None)
def _centred_reference(kind):
    x = _forms(_centred_inputs(), "cpu")[kind]
    mu = x.to(torch.float64).mean(dim=0)
    Xc = _staged(x, mu)
    w, V = np.linalg.eigh(Xc.T @ Xc / Xc.shape[0])
    return mu, w[-4:], V[:, -4:], w


@pytest.mark.parametrize("kind", ("u8", "f32", "bf16"))
def test_centred_samples(kind, cuda):
    import distributed_eigenspaces_amd as de
    x = _forms(_centred_inputs(), cuda)[kind]
    mu, w, V, _ = _centred_reference(kind)
    _check(de.topk_samples(x, 4, center=mu), V, w)


@functools.lru_cache(maxsize=None)
def _wide_inputs():
    Xq, _ = spiked_int_data(384, 40960, 4, seed=13, theta_hi=4000, theta_lo=2000)
    assert Xq.min() >= -128 and Xq.max() <= 127  # none clip
    return Xq


@pytest.mark.parametrize("kind", ("u8", "bf16"))
def test_beyond_the_explicit_routes_reach(kind, cuda):
    """d = 40960 > 32768, n = 384: the reference is the 384 x 384 dual Gram in float64."""
    import distributed_eigenspaces_amd as de
    Xq = _wide_inputs()
    x = _forms(Xq, "cpu")[kind]
    mu = x.to(torch.float64).mean(dim=0)
    Xc = _staged(x, mu)
    n = Xc.shape[0]
    w, Uu = np.linalg.eigh(Xc @ Xc.T / n)
    V = Xc.T @ Uu[:, -4:]
    V /= np.linalg.norm(V, axis=0)
    _check(de.topk_samples(x.to(cuda), 4, center=mu), V, w[-4:])


def test_warm_start_and_sweep_budget(cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd import _lib
    x = _forms(_centred_inputs(), cuda)["f32"]
    mu, w, V, _ = _centred_reference("f32")
    cold = de.topk_samples(x, 4, center=mu)
    warm = de.topk_samples(x, 4, center=mu, q0=cold.V)
    _check(warm, V, w)
    assert warm.sweeps < cold.sweeps
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r = de.topk_samples(x, 4, center=mu, max_sweeps=1)
    assert not r.converged
    assert any(issubclass(m.category, _lib.NotConvergedWarning) for m in rec)


def test_estimator_free_route_golden(cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    g = load_golden("spiked_d256_k10_m8")
    k = int(g["k"])
    assert int(g["m"]) == 8
    X = torch.from_numpy(g["X"].astype(np.float32)).to(cuda)
    r = DistributedEigenspaceEstimator(k, workers_per_rank=8, covariance="free").fit(X)
    assert ref_cpu.projector_distance(r.V.cpu().numpy(), g["server_V"]) <= P_TOL
    np.testing.assert_allclose(r.evals.cpu().numpy(), g["server_evals"], rtol=EV_TOL)
    assert de.topk_samples is de.linalg.topk_samples


def test_pca_free_route_bytes(cuda):
    """PCA(4, covariance="free", u8_mode="raw") on the 1500 x 132 bytes against float64 NumPy
    PCA, with test_gpu_pca.py's tolerances."""
    from distributed_eigenspaces_amd.pca import PCA
    x = _forms(_centred_inputs(), cuda)["u8"]
    mu, w, V, wall = _centred_reference("u8")
    N = x.shape[0]
    p = PCA(4, covariance="free", u8_mode="raw").fit(x)
    assert p.mean_.dtype == torch.float64
    np.testing.assert_allclose(p.mean_.cpu().numpy(), mu.numpy(), rtol=1e-12)
    comp = p.components_.cpu().numpy()
    assert ref_cpu.projector_distance(comp.T, V) <= P_TOL
    np.testing.assert_allclose(p.explained_variance_.cpu().numpy(), w[::-1] * N / (N - 1), rtol=EV_TOL)
    np.testing.assert_allclose(p.explained_variance_ratio_.cpu().numpy(), w[::-1] / wall.sum(),
                               atol=1e-5, rtol=0)
    np.testing.assert_allclose(comp @ comp.T, np.eye(4), atol=1e-5)
