"""Procrustes-aligned basis averaging (linalg.procrustes_average) and the residual-form
subspace distance (linalg.subspace_distance) against a float64 restatement in numpy.

The restatement, from the fp32 inputs the GPU saw:
  G_i = V_i^T R;  U, c, W^T = svd(G_i);  Z_i = sum_{c_j > 1e-5 c_max} u_j w_j^T;
  Vbar = sum_i w_i V_i Z_i;  V = Vbar (Vbar^T Vbar)^(-1/2).
Bars: the project's P_TOL (1e-4), EV_TOL (1e-5) and orthonormality (1e-5) bars.
"""
import functools
import os

import numpy as np
import pytest
import torch

import distributed_eigenspaces_amd as de
from distributed_eigenspaces_amd import _lib
from oracle import ref_cpu
from tests.conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

P_TOL = 1e-4
EV_TOL = 1e-5
ORTH_TOL = 1e-5
MIN_COS = 0.25  # the well-posed regime every parity input is asserted to be in

SHAPES = [(64, 3, 5), (250, 7, 3), (256, 10, 8), (512, 17, 8), (1024, 64, 8), (2048, 128, 4),
          (64, 1, 4), (16, 16, 3)]


# ---------------------------------------------------------------- float64 restatement
def restate(Vs, R, w=None, iters=1):
    """Vs: (m, d, k) float64, R: (d, k).  Returns V, Z (m, k, k), cosines (m, k) of the last
    pass and the smallest cosine of the first pass."""
    m = Vs.shape[0]
    w = np.full(m, 1.0 / m) if w is None else np.asarray(w, np.float64) / np.sum(w)
    first_min = None
    for _ in range(iters):
        Zs, cs = [], []
        Vbar = np.zeros_like(R)
        for i in range(m):
            U, c, Wt = np.linalg.svd(Vs[i].T @ R)
            keep = c > 1e-5 * c.max()
            Z = U[:, keep] @ Wt[keep]
            Zs.append(Z)
            cs.append(c)
            Vbar += w[i] * (Vs[i] @ Z)
        if first_min is None:
            first_min = min(float(c.min()) for c in cs)
        lam, Q = np.linalg.eigh(Vbar.T @ Vbar)
        R = Vbar @ ((Q / np.sqrt(lam)) @ Q.T)
    return R, np.stack(Zs), np.stack(cs), first_min


def qf(a):
    """Q factor with a positive diagonal of R (a continuous function of a)."""
    q, r = np.linalg.qr(a)
    s = np.sign(np.diag(r))
    s[s == 0] = 1.0
    return q * s


@functools.lru_cache(maxsize=None)
def planted_inputs(d, k, m, eps, seed=1):
    """V_i = qr(U + eps / sqrt(d) N_i) qr(M_i) as fp32 (m, d, k), and the planted U."""
    rng = np.random.default_rng(seed)
    U = qf(rng.standard_normal((d, k)))
    Vs = np.stack([qf(U + eps / np.sqrt(d) * rng.standard_normal((d, k)))
                   @ qf(rng.standard_normal((k, k))) for _ in range(m)]).astype(np.float32)
    Vs.flags.writeable = False
    U.flags.writeable = False
    return Vs, U


def gpu_average(Vs32, k, cuda, **kw):
    Wt = de.stack_bases([torch.from_numpy(np.array(v)).to(cuda) for v in Vs32])
    r = de.procrustes_average(Wt, k, **kw)
    torch.cuda.synchronize()
    return r.V.cpu().numpy().astype(np.float64), r.Z.cpu().numpy(), r.cosines.cpu().numpy(), Wt


def check_parity(Vs32, k, cuda, ref=None, weights=None, iters=1, ref_arg=None):
    Vs = Vs32.astype(np.float64)
    R = Vs[0] if ref is None else ref
    V64, Z64, c64, min_cos = restate(Vs, R, weights, iters)
    assert min_cos >= MIN_COS, f"ill-posed test input: smallest cosine {min_cos}"
    kw = {}
    if ref_arg is not None:
        kw["ref"] = ref_arg
    if weights is not None:
        kw["weights"] = weights
    if iters != 1:
        kw["iters"] = iters
    V, Z, c, _ = gpu_average(Vs32, k, cuda, **kw)
    dP = ref_cpu.projector_distance(V, V64)
    dV = np.linalg.norm(V - V64)
    orth = np.max(np.abs(V.T @ V - np.eye(k)))
    dc = np.max(np.abs(c - c64))
    dZ = max(np.linalg.norm(Vs[i] @ Z[i] - Vs[i] @ Z64[i]) for i in range(len(Vs)))
    print(f"dP={dP:.2e} dV={dV:.2e} orth={orth:.2e} dcos={dc:.2e} dZ={dZ:.2e} mincos={min_cos:.3f}")
    assert np.isfinite(V).all()
    assert dP <= P_TOL
    assert dV <= P_TOL  # pins the rotation inside the span, not only the span
    assert orth <= ORTH_TOL
    assert dc <= EV_TOL
    assert dZ <= P_TOL
    assert np.all(np.diff(c, axis=1) <= 0), "cosines must be descending"


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("eps", [0.3, 1.0])
@pytest.mark.parametrize("d,k,m", SHAPES)
def test_parity(cuda, d, k, m, eps):
    Vs32, _ = planted_inputs(d, k, m, eps)
    check_parity(Vs32, k, cuda)


@pytest.mark.parametrize("d,k,m", SHAPES)
def test_parity_two_passes(cuda, d, k, m):
    Vs32, _ = planted_inputs(d, k, m, 0.3)
    check_parity(Vs32, k, cuda, iters=2)


@pytest.mark.parametrize("d,k,m", SHAPES)
def test_parity_unequal_weights(cuda, d, k, m):
    Vs32, _ = planted_inputs(d, k, m, 0.3)
    check_parity(Vs32, k, cuda, weights=[1.0 + 0.5 * i for i in range(m)])


@pytest.mark.parametrize("d,k,m", SHAPES)
def test_parity_explicit_reference(cuda, d, k, m):
    """ref as a tensor (the planted basis, not a member of the stack) and as an index."""
    Vs32, U = planted_inputs(d, k, m, 0.3)
    U32 = U.astype(np.float32)
    check_parity(Vs32, k, cuda, ref=U32.astype(np.float64), ref_arg=torch.from_numpy(U32).to(cuda))
    check_parity(Vs32, k, cuda, ref=Vs32[m - 1].astype(np.float64), ref_arg=m - 1)


# ---------------------------------------------------------------- exact cases
def signed_permutations(k, m, seed=3):
    rng = np.random.default_rng(seed)
    out = [np.eye(k)]
    for _ in range(m - 1):
        P = np.eye(k)[:, rng.permutation(k)] * rng.choice([-1.0, 1.0], size=k)
        out.append(P)
    return out


def test_signed_permutations_are_undone(cuda):
    d, k, m = 96, 6, 4
    V1 = qf(np.random.default_rng(2).standard_normal((d, k))).astype(np.float32)
    PDs = signed_permutations(k, m)
    Vs32 = np.stack([(V1 @ PD.astype(np.float32)) for PD in PDs])  # exact in fp32
    V, Z, c, _ = gpu_average(Vs32, k, cuda)
    assert np.max(np.abs(V - V1)) <= 1e-6
    for i in range(m):
        assert np.max(np.abs(Z[i] - PDs[i].T)) <= 1e-6
    assert np.max(np.abs(c - 1.0)) <= 1e-6


def test_single_basis_returns_it(cuda):
    d, k = 96, 6
    V1 = qf(np.random.default_rng(4).standard_normal((d, k))).astype(np.float32)
    V, _, _, _ = gpu_average(V1[None], k, cuda)
    assert np.max(np.abs(V - V1)) <= 1e-6


def test_unit_weight_returns_first_span(cuda):
    Vs32, _ = planted_inputs(256, 10, 8, 0.3)
    V, _, _, _ = gpu_average(Vs32, 10, cuda, weights=[1.0] + [0.0] * 7)
    assert ref_cpu.projector_distance(V, Vs32[0]) <= 1e-6


# ---------------------------------------------------------------- why alignment matters
def test_alignment_beats_worker_and_naive_mean(cuda):
    Vs32, U = planted_inputs(256, 10, 8, 0.3)
    V, _, _, _ = gpu_average(Vs32, 10, cuda)
    worker1 = ref_cpu.projector_distance(Vs32[0], U)
    got = ref_cpu.projector_distance(V, U)
    naive = ref_cpu.projector_distance(qf(Vs32.astype(np.float64).mean(axis=0)), U)
    print(f"procrustes {got:.4f}  worker1 {worker1:.4f}  naive mean {naive:.4f}")
    assert got < 0.6 * worker1  # float64 restatement: 0.36 x
    assert naive > worker1


# ---------------------------------------------------------------- degenerate cosine
def test_degenerate_cosine(cuda):
    """One basis has a column exactly orthogonal to the reference span: finite result,
    that cosine ~ 0, its direction contributes nothing."""
    d, k, m = 64, 4, 3
    rng = np.random.default_rng(7)
    V1 = np.zeros((d, k))
    V1[:32] = qf(rng.standard_normal((32, k)))  # the reference lives on coordinates 0..31
    V2 = qf(V1 + 0.3 / np.sqrt(d) * rng.standard_normal((d, k)))
    N = np.zeros((d, 3))
    N[:40] = rng.standard_normal((40, 3))
    V3 = np.zeros((d, k))
    V3[:, :3] = qf(V1[:, :3] + 0.3 / np.sqrt(d) * N)  # zero on coordinate 40
    V3[40, 3] = 1.0                                    # exactly orthogonal to span(V1)
    Vs32 = np.stack([V1, V2, V3]).astype(np.float32)
    assert np.all(Vs32[2][:, 3] @ Vs32[0] == 0.0)
    V, Z, c, _ = gpu_average(Vs32, k, cuda)
    V64, _, _, _ = restate(Vs32.astype(np.float64), Vs32[0].astype(np.float64))
    assert np.isfinite(V).all() and np.isfinite(Z).all() and np.isfinite(c).all()
    assert np.max(np.abs(V.T @ V - np.eye(k))) <= ORTH_TOL
    assert c[2, -1] <= 1e-5
    assert ref_cpu.projector_distance(V, V64) <= P_TOL


# ---------------------------------------------------------------- the reference's golden server
@pytest.mark.parametrize("name", ["spiked_d64_k4_m8", "spiked_d128_k2_m5_ragged",
                                  "spiked_d256_k10_m8", "spiked_d256_k16_m4"])
def test_close_to_golden_server(cuda, name):
    g = load_golden(name)
    k = int(g["k"])
    Wt = de.stack_bases(list(g["worker_V"]))
    V = de.procrustes_average(Wt, k).V.cpu().numpy()
    nearest = min(ref_cpu.projector_distance(w, g["server_V"]) for w in g["worker_V"])
    got = ref_cpu.projector_distance(V, g["server_V"])
    print(f"{name}: {got:.4f} vs nearest worker {nearest:.4f} (ratio {got / nearest:.4f})")
    assert got <= 0.05 * nearest  # float64 restatement: <= 0.0175


def test_two_bases_give_the_golden_span(cuda):
    """m = 2, equal weights: the bisector subspace is both aggregators' answer."""
    # the stored bases only: the fixture's samples (regenerated from its seed) are not needed
    with np.load(os.path.join(GOLDEN, "spiked_d3072_k16_m2_seeded.npz"), allow_pickle=False) as z:
        wv, sv, k = z["worker_V"], z["server_V"], int(z["k"])
    V = de.procrustes_average(de.stack_bases(list(wv)), k).V.cpu().numpy()
    assert ref_cpu.projector_distance(V, sv) <= P_TOL


# ---------------------------------------------------------------- estimator / streaming
def test_estimator_procrustes_aggregate(cuda):
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    g = load_golden("spiked_d256_k10_m8")
    k, m = int(g["k"]), int(g["m"])
    X = torch.from_numpy(g["X"].astype(np.float32)).to(cuda)
    res = DistributedEigenspaceEstimator(k, workers_per_rank=8, aggregate="procrustes").fit(X)
    torch.cuda.synchronize()
    assert res.evals is None and res.sweeps_server == 0
    assert res.cosines is not None and tuple(res.cosines.shape) == (m, k)
    Vs = res.Wt.cpu().numpy().astype(np.float64).reshape(m, k, -1).transpose(0, 2, 1)
    V64, _, c64, _ = restate(Vs, Vs[0])
    assert ref_cpu.projector_distance(res.V.cpu().numpy(), V64) <= P_TOL
    assert np.max(np.abs(res.cosines.cpu().numpy() - c64)) <= EV_TOL
    # the default aggregate is untouched: same call without the argument is the projector server
    dflt = DistributedEigenspaceEstimator(k, workers_per_rank=8).fit(X)
    assert dflt.cosines is None and dflt.evals is not None and dflt.sweeps_server > 0
    with pytest.raises(ValueError):
        DistributedEigenspaceEstimator(k, aggregate="mean")


def test_streaming_procrustes_keeps_columns(cuda):
    from distributed_eigenspaces_amd import synthetic
    from distributed_eigenspaces_amd.streaming import StreamingOja
    d, k, b, agg, eta = 256, 6, 1024, 4, 0.3
    U = synthetic.planted_basis(d, k, seed=5, device=cuda)
    X = synthetic.spiked_samples(2 * agg * b, U, seed=6)
    V0 = torch.linalg.qr(torch.randn(d, k, device=cuda, dtype=torch.float64))[0].float()
    s = StreamingOja(V0, eta=eta, agg_every=0, aggregate="procrustes")  # aggregate by hand
    for j in range(2):  # Oja steps, then an aggregation, twice
        s.partial_fit_block(X[j * agg * b:(j + 1) * agg * b], b)
        before = s.V.clone()
        s.aggregate()
        diag = torch.diagonal(s.V.t() @ before).cpu().numpy()
        print("diag(V_after^T V_before) =", np.round(diag, 6))
        assert np.all(np.sign(diag) == 1.0) and np.all(np.abs(diag) > 0.9)
    assert s.aggregations == 2
    Vg = s.V.cpu().numpy()
    np.testing.assert_allclose(Vg.T @ Vg, np.eye(k), atol=ORTH_TOL)
    assert StreamingOja(V0, eta=eta).aggregator == "projector"  # default unchanged


# ---------------------------------------------------------------- subspace distance
@functools.lru_cache(maxsize=None)
def distance_inputs(d, k, eps, seed=11):
    rng = np.random.default_rng(seed)
    A = qf(rng.standard_normal((d, k)))
    B = qf(A + eps / np.sqrt(d) * rng.standard_normal((d, k))) @ qf(rng.standard_normal((k, k)))
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    A64, B64 = A32.astype(np.float64), B32.astype(np.float64)
    R = B64 - A64 @ (A64.T @ B64)
    return A32, B32, float(np.linalg.norm(R)), float(np.linalg.norm(R, 2))


@pytest.mark.parametrize("eps", [0.0, 1e-6, 1e-4, 1e-2, 0.5])
@pytest.mark.parametrize("d,k", [(64, 3), (1000, 37), (2048, 128)])
def test_subspace_distance(cuda, d, k, eps):
    A32, B32, fro64, two64 = distance_inputs(d, k, eps)
    A, B = torch.from_numpy(A32.copy()).to(cuda), torch.from_numpy(B32.copy()).to(cuda)
    fro, two = de.subspace_distance(A, B)
    pd = de.projector_distance(A, B)
    pd64 = ref_cpu.projector_distance(A32, B32)
    print(f"fro {fro:.6e} / {fro64:.6e}  two {two:.6e} / {two64:.6e}  proj {pd:.6e} / {pd64:.6e}")
    assert abs(fro - fro64) <= 1e-5 + 1e-5 * fro64
    assert abs(two - two64) <= 1e-5 + 1e-5 * two64
    assert abs(pd - pd64) <= 1e-5 + 1e-5 * pd64


# ---------------------------------------------------------------- hygiene
def test_bit_identical_and_input_untouched(cuda):
    Vs32, _ = planted_inputs(512, 17, 8, 1.0)
    V1, Z1, c1, Wt = gpu_average(Vs32, 17, cuda)
    Wt0 = Wt.clone()
    r = de.procrustes_average(Wt, 17)
    torch.cuda.synchronize()
    assert np.array_equal(r.V.cpu().numpy().astype(np.float64), V1)
    assert np.array_equal(r.Z.cpu().numpy(), Z1)
    assert np.array_equal(r.cosines.cpu().numpy(), c1)
    assert torch.equal(Wt, Wt0)


@pytest.mark.parametrize("d,k,m", [(2048, 128, 4), (250, 7, 3)])
def test_workspace_canary(cuda, d, k, m):
    """A workspace of exactly the queried size, followed by a canary."""
    Vs32, _ = planted_inputs(d, k, m, 0.3)
    dp = (d + 3) // 4 * 4
    Wt = torch.zeros((m * k, dp), dtype=torch.float32, device=cuda)
    Wt[:, :d] = torch.from_numpy(np.ascontiguousarray(Vs32.transpose(0, 2, 1)).reshape(m * k, d)).to(cuda)
    L = _lib.lib()
    CAN = 4096
    with torch.cuda.device(cuda):
        nbytes = L.deig_procrustes_workspace(dp, m * k, k)
        ws = torch.full((nbytes + CAN,), 0xA5, dtype=torch.uint8, device=cuda)
        V = torch.empty((k, dp), dtype=torch.float32, device=cuda)
        Z = torch.empty((m, k, k), dtype=torch.float32, device=cuda)
        c = torch.empty((m, k), dtype=torch.float32, device=cuda)
        st = torch.cuda.current_stream(cuda).cuda_stream
        rc = L.deig_procrustes_avg_f32(Wt.data_ptr(), dp, m * k, dp, k, None, dp, None, 1,
                                       V.data_ptr(), dp, Z.data_ptr(), c.data_ptr(), ws.data_ptr(),
                                       nbytes, st)
        assert rc == _lib.DEIG_OK, _lib.last_error()
        rc = L.deig_procrustes_avg_f32(Wt.data_ptr(), dp, m * k, dp, k, None, dp, None, 1,
                                       V.data_ptr(), dp, Z.data_ptr(), c.data_ptr(), ws.data_ptr(),
                                       nbytes - 1, st)
        assert rc == _lib.DEIG_EWORKSPACE
        nd = L.deig_subspace_dist_workspace(dp, k)
        wsd = torch.full((nd + CAN,), 0xA5, dtype=torch.uint8, device=cuda)
        out = torch.empty(2, dtype=torch.float32, device=cuda)
        rc = L.deig_subspace_dist_f32(V.data_ptr(), dp, Wt.data_ptr(), dp, dp, k, out.data_ptr(),
                                      wsd.data_ptr(), nd, st)
        assert rc == _lib.DEIG_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "procrustes wrote past its workspace"
    assert bool((wsd[nd:] == 0xA5).all()), "subspace_dist wrote past its workspace"
    Vg = V.t()[:d].cpu().numpy().astype(np.float64)
    V64, _, _, _ = restate(Vs32.astype(np.float64), Vs32[0].astype(np.float64))
    assert ref_cpu.projector_distance(Vg, V64) <= P_TOL
    assert np.isfinite(out.cpu().numpy()).all()
