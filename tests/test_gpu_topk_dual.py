"""The wide-data worker solve through the n x n Gram matrix of the samples (linalg.topk_dual,
deig_topk_dual) and the routes built on it: DistributedEigenspaceEstimator(covariance="dual")
and PCA(covariance="dual").

The bars are the project's (test_gpu_pipeline.py): ||P - P_ref||_F <= 1e-4 and eigenvalues to
1e-5 relative, always against float64 references - the reference run's golden outputs, or
NumPy on the staged matrix Xc = fl32((double)x - c) - never against another GPU route."""
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
KINDS = ("u8", "f32", "bf16")


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


def _forms(Xq, dev):
    return {"u8": torch.from_numpy((Xq + 128).astype(np.uint8)).to(dev),
            "f32": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev),
            "bf16": torch.from_numpy(Xq.astype(np.float32) / 8).to(dev).to(torch.bfloat16)}


@pytest.mark.parametrize("name", ["spiked_d256_k10_m8", "spiked_d64_k4_m8"])
def test_golden_workers(name, cuda):
    """Every shard's topk_dual against the reference run's worker outputs (zero-mean data;
    the shards have more rows than features, which is legal: K then has rank d)."""
    import distributed_eigenspaces_amd as de
    g = load_golden(name)
    k = int(g["k"])
    X = torch.from_numpy(g["X"].astype(np.float32)).to(cuda)
    for i, (lo, hi) in enumerate(np.asarray(g["ranges"]).reshape(-1, 2)):
        r = de.topk_dual(X[int(lo):int(hi)], k)
        _check(r, g["worker_V"][i], np.sort(np.asarray(g["worker_evals"][i], dtype=np.float64)))


# (n, d, k, seed, theta_hi, theta_lo): the tall case (K of rank <= d), d beyond the explicit
# route, a ragged small n (not a multiple of 4 or 16; gap ratio lambda_4 / lambda_3 = 0.28) and
# an inner dimension past the 16384 flush limit (gap ratio 0.14).  No value clips.
INPUTS = {"tall": (1500, 132, 4, 11, 8.0, 4.0), "wide": (384, 40960, 4, 13, 4000, 2000),
          "ragged": (50, 2056, 3, 17, 400, 200), "long": (130, 16424, 4, 19, 2000, 1000)}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    n, d, k, seed, hi, lo = INPUTS[name]
    Xq, _ = spiked_int_data(n, d, k, seed=seed, theta_hi=hi, theta_lo=lo)
    assert Xq.min() >= -128 and Xq.max() <= 127  # none clip
    return Xq


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """(column mean, top-k evals ascending, top-k vectors, all evals) in float64; through the
    n x n dual Gram where n < d."""
    k = INPUTS[name][2]
    x = _forms(_inputs(name), "cpu")[kind]
    mu = x.to(torch.float64).mean(dim=0)
    Xc = _staged(x, mu)
    n, d = Xc.shape
    if n >= d:
        w, V = np.linalg.eigh(Xc.T @ Xc / n)
        return mu, w[-k:], V[:, -k:], w
    w, Uu = np.linalg.eigh(Xc @ Xc.T / n)
    V = Xc.T @ Uu[:, -k:]
    V /= np.linalg.norm(V, axis=0)
    return mu, w[-k:], V, w


CASES = [(name, kind) for name in ("tall", "wide", "ragged") for kind in KINDS] + \
        [("long", "bf16"), ("long", "u8")]


@pytest.mark.parametrize("name,kind", CASES)
def test_centred_samples(name, kind, cuda):
    import distributed_eigenspaces_amd as de
    x = _forms(_inputs(name), cuda)[kind]
    mu, w, V, _ = _reference(name, kind)
    _check(de.topk_dual(x, INPUTS[name][2], center=mu), V, w)


@pytest.mark.parametrize("kind", KINDS)
def test_the_start_is_worth_having(kind, cuda):
    """The finish from the dual start takes fewer sweeps than topk_samples from a cold start."""
    import distributed_eigenspaces_amd as de
    x = _forms(_inputs("wide"), cuda)[kind]
    mu = _reference("wide", kind)[0]
    dual, cold = de.topk_dual(x, 4, center=mu), de.topk_samples(x, 4, center=mu)
    print(f"finish sweeps {dual.sweeps}, cold sweeps {cold.sweeps}")
    assert dual.converged and cold.converged
    assert dual.sweeps < cold.sweeps


def test_sweep_budget(cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd import _lib
    x = _forms(_inputs("tall"), cuda)["f32"]
    mu = _reference("tall", "f32")[0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r = de.topk_dual(x, 4, center=mu, max_sweeps=1)
    assert not r.converged
    assert any(issubclass(m.category, _lib.NotConvergedWarning) for m in rec)


def test_estimator_dual_route_golden(cuda):
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    g = load_golden("spiked_d256_k10_m8")
    k = int(g["k"])
    assert int(g["m"]) == 8
    X = torch.from_numpy(g["X"].astype(np.float32)).to(cuda)
    r = DistributedEigenspaceEstimator(k, workers_per_rank=8, covariance="dual").fit(X)
    assert ref_cpu.projector_distance(r.V.cpu().numpy(), g["server_V"]) <= P_TOL
    np.testing.assert_allclose(r.evals.cpu().numpy(), g["server_evals"], rtol=EV_TOL)


def test_pca_dual_route_bytes(cuda):
    """PCA(4, covariance="dual", u8_mode="raw") on the 1500 x 132 bytes against float64 NumPy
    PCA, with test_gpu_pca.py's tolerances."""
    from distributed_eigenspaces_amd.pca import PCA
    x = _forms(_inputs("tall"), cuda)["u8"]
    mu, w, V, wall = _reference("tall", "u8")
    N = x.shape[0]
    p = PCA(4, covariance="dual", u8_mode="raw").fit(x)
    assert p.mean_.dtype == torch.float64
    np.testing.assert_allclose(p.mean_.cpu().numpy(), mu.numpy(), rtol=1e-12)
    comp = p.components_.cpu().numpy()
    assert ref_cpu.projector_distance(comp.T, V) <= P_TOL
    np.testing.assert_allclose(p.explained_variance_.cpu().numpy(), w[::-1] * N / (N - 1), rtol=EV_TOL)
    np.testing.assert_allclose(p.explained_variance_ratio_.cpu().numpy(), w[::-1] / wall.sum(),
                               atol=1e-5, rtol=0)
    np.testing.assert_allclose(comp @ comp.T, np.eye(4), atol=1e-5)
