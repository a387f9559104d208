"""The GPU top_k_eigenvectors is as general as the reference's (distributed.py:22-29:
``scipy.linalg.eigh(matrix, eigvals=(N-k, N-1))`` - any symmetric matrix, any
1 <= k <= N): k > 128 (block locking, csrc/solver.hip SolveSM) and indefinite input
(detected from the Ritz values, solved as S + sigma I), for explicit float32 /
float64 matrices and for the implicit projector average (server, k > 128).

Matrices have a planted spectrum S = U diag(lambda) U^T with a clear gap at k (the
bar ||P - P_ref||_F <= 1e-4 needs residual / gap << 1e-4; internal block boundaries
need no gap), plus a GOE matrix (no planted structure, |lambda_min| ~ lambda_max) at
k where its own gap allows the bar.  Bars: ||P - P_ref||_F <= 1e-4, eigenvalues
1e-5 relative (north_star), against ref_cpu.top_k_eigh (the reference's eigh call)."""
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
P_TOL, EV_TOL = 1e-4, 1e-5


def planted(d, lam, seed, device):
    """U diag(lam) U^T in float64 on the GPU (U from a QR of a Gaussian), and on host."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = torch.randn(d, d, generator=g, dtype=torch.float64).to(device)
    U, _ = torch.linalg.qr(A)
    S = (U * torch.as_tensor(lam, dtype=torch.float64, device=device)) @ U.t()
    S = 0.5 * (S + S.t())
    return S, S.cpu().numpy()


def spectrum(d, k, top=(10.0, 5.0), rest=(2.0, 0.0)):
    return np.concatenate([np.linspace(top[0], top[1], k), np.linspace(rest[0], rest[1], d - k)])


def check(r, S_h, k, p_tol=P_TOL, ev_tol=EV_TOL):
    w, V = ref_cpu.top_k_eigh(S_h, k)
    assert r.converged
    got_w = r.evals.double().cpu().numpy()
    assert np.all(np.diff(got_w) >= -1e-6 * np.abs(got_w).max())  # ascending
    assert ref_cpu.projector_distance(r.V.cpu().numpy(), V) <= p_tol
    np.testing.assert_allclose(got_w, w, rtol=ev_tol, atol=ev_tol * np.abs(w).max() * 1e-2)


@pytest.mark.parametrize("d,k,dtype", [(1024, 200, torch.float32), (3072, 256, torch.float64),
                                       (1024, 129, torch.float64), (512, 512, torch.float64)])
def test_k_above_128_block_locking(d, k, dtype, cuda):
    """k > 128: blocks of 112 pairs on a 128-column subspace, locked and deflated
    (k = d: every eigenpair)."""
    import distributed_eigenspaces_amd as de
    lam = spectrum(d, k) if k < d else np.linspace(10.0, 1.0, d)
    S, S_h = planted(d, lam, seed=d + k, device=cuda)
    r = de.topk_eigh(S.to(dtype), k)
    check(r, S.to(dtype).double().cpu().numpy(), k)


def test_k_above_128_node_api_numpy(cuda):
    """The drop-in Node.top_k_eigenvectors (numpy float64 in / out) at k = 200."""
    from distributed_eigenspaces_amd import distributed as dd
    d, k = 1024, 200
    _, S_h = planted(d, spectrum(d, k), seed=7, device=cuda)
    V = dd.top_k_eigenvectors(S_h, k)
    assert isinstance(V, np.ndarray) and V.shape == (d, k) and V.flags["F_CONTIGUOUS"]
    assert ref_cpu.projector_distance(V, ref_cpu.top_k_eigenvectors(S_h, k)) <= P_TOL


@pytest.mark.parametrize("case", ["negative_bulk_dominates", "negative_definite", "mixed_k150"])
def test_indefinite_planted(case, cuda):
    """Indefinite S: the top-k ALGEBRAIC pairs even when |lambda_min| > lambda_1."""
    import distributed_eigenspaces_amd as de
    d = 768
    if case == "negative_bulk_dominates":
        k, lam = 10, np.concatenate([np.linspace(10, 6, 10), np.linspace(2, -1, d - 20),
                                     np.linspace(-20, -30, 10)])
    elif case == "negative_definite":
        k, lam = 8, np.concatenate([np.linspace(-1, -2, 8), np.linspace(-4, -50, d - 8)])
    else:
        k, lam = 150, np.concatenate([np.linspace(5, 3, 150), np.linspace(1, -8, d - 150)])
    seed = {"negative_bulk_dominates": 11, "negative_definite": 12, "mixed_k150": 13}[case]
    S, S_h = planted(d, lam, seed=seed, device=cuda)
    r = de.topk_eigh(S.float(), k)
    check(r, S.float().double().cpu().numpy(), k)


@pytest.mark.parametrize("k", [1, 5])
def test_indefinite_goe(k, cuda):
    """A GOE matrix (A + A^T)/sqrt(2d): semicircle on [-2, 2], lambda_min ~ -lambda_max;
    k where its own top gap (4.3 % / 2.5 % of lambda_max, seed 1) allows the bar."""
    import distributed_eigenspaces_amd as de
    d = 256
    rng = np.random.default_rng(1)
    A = rng.standard_normal((d, d))
    S_h = (A + A.T) / np.sqrt(2 * d)
    r = de.topk_eigh(torch.from_numpy(S_h).to(cuda), k, tol=1e-7)
    check(r, S_h, k)


def test_projector_average_k_above_128(cuda):
    """Server solve with k = 160 > 128: the implicit operator scale * Wt^T Wt with the
    locked pairs deflated by products (d x d never formed), vs eigh of the explicit
    average (distributed.py:126-130 + NB:306).  Four workers share k - 8 directions
    (eigenvalue 1), three of them 8 more (0.75), the fourth 8 private ones (0.25):
    the top-k subspace is unique; each basis is scrambled by a random rotation."""
    import distributed_eigenspaces_amd as de
    d, k, m = 1024, 160, 4
    g = torch.Generator(device="cpu").manual_seed(3)
    Q = torch.linalg.qr(torch.randn(d, k + 8, generator=g, dtype=torch.float64))[0]
    common, shared, private = Q[:, :k - 8], Q[:, k - 8:k], Q[:, k:]
    bases = []
    for i in range(m):
        B = torch.cat([common, shared if i < 3 else private], dim=1)
        R = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64))[0]
        bases.append(B @ R)
    Vs = [b.cpu().numpy() for b in bases]
    w, V = ref_cpu.server_topk(Vs, k, m)
    Wt = de.linalg.stack_bases([b.float().to(cuda) for b in bases])
    r = de.linalg.projavg_topk(Wt, k, 1.0 / m)
    assert r.converged
    Pd = ref_cpu.projector_distance(r.V.cpu().numpy(), V)
    assert Pd <= P_TOL, Pd
    np.testing.assert_allclose(r.evals.double().cpu().numpy(), w, rtol=EV_TOL, atol=1e-6)


@pytest.mark.parametrize("d,k,case", [(766, 5, "negative_definite"), (766, 12, "mixed"),
                                      (10, 3, "negative_definite"), (13, 4, "mixed"),
                                      (20, 18, "negative_definite")])
def test_indefinite_padded_dimension(d, k, case, cuda):
    """d % 4 != 0 or d < 16 (the library stages S in a zero-padded copy): the padding's
    eigenvalue-0 directions must not outrank S's own negative top-k eigenpairs (r03
    padded in Python and returned them as converged zero columns).  d = 766:
    the start basis has zero padding rows; d = 10 / 13 / 20: the basis spans the padded
    space, whose diagonal is set below S's spectrum."""
    import distributed_eigenspaces_amd as de
    if case == "negative_definite":  # a clear gap below the top k, like the other planted cases
        lam = -np.concatenate([np.linspace(1.0, 2.0, k), np.linspace(4.0, 40.0, d - k)])
    else:  # top k straddle zero, most of the spectrum negative
        lam = np.concatenate([np.linspace(2.0, 1.0, k // 2), -np.linspace(0.5, 1.5, k - k // 2),
                              -np.linspace(3.0, 30.0, d - k)])
    S, S_h = planted(d, lam, seed=d + k, device=cuda)
    r = de.topk_eigh(S.float(), k)
    assert r.V.shape == (d, k)
    check(r, S.float().double().cpu().numpy(), k)
    Vh = r.V.double().cpu().numpy()
    np.testing.assert_allclose(Vh.T @ Vh, np.eye(k), atol=1e-5)
    # the float64 S and the batched solver take the same staging
    r64 = de.topk_eigh(S, k)
    check(r64, S_h, k)
    rb = de.topk_eigh_batch([S.float(), S.float()], k)
    for x in rb:
        check(x, S.float().double().cpu().numpy(), k)


def test_batch_status_is_per_problem(cuda):
    """One batched solve of an easy and an impossible problem (gap 0.999, 40 sweeps):
    each result's converged flag is that problem's own outcome (one
    unconverged problem used to mark every problem unconverged)."""
    import warnings

    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd import _lib
    d, k = 512, 8
    easy, _ = planted(d, spectrum(d, k), seed=21, device=cuda)
    hard, _ = planted(d, np.concatenate([np.linspace(2.0, 1.0, k), np.linspace(0.999, 0.5, d - k)]),
                      seed=22, device=cuda)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        rs = de.topk_eigh_batch([easy.float(), hard.float()], k, max_sweeps=40)
    assert any(issubclass(x.category, _lib.NotConvergedWarning) for x in rec)
    assert rs[0].converged and not rs[1].converged
    single = de.topk_eigh(easy.float(), k, max_sweeps=40)
    assert torch.equal(single.V, rs[0].V) and torch.equal(single.evals, rs[0].evals)


def test_k_above_128_rank_deficient(cuda):
    """k = 200 > 128 on a rank-100 PSD covariance (n = 100 rows, d = 512): the second
    block's pairs are S's null space, where the deflated locked pairs (~0) compete; V
    must stay orthonormal, the top-100 subspace match eigh, the null
    pairs' eigenvalues be ~0 and every residual small.  And the solve must END cleanly
    like ?syevr (distributed.py:29): the null block is judged by its residual against
    |lambda_max| (include/deig.h), not against its own ~0 Ritz values - r04 burned
    ~300 sweeps there and warned NotConverged on a correct answer."""
    import distributed_eigenspaces_amd as de
    d, n, k, rank = 512, 100, 200, 100
    g = torch.Generator(device="cpu").manual_seed(5)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    X *= torch.linspace(3.0, 1.0, d, dtype=torch.float64)  # a spread spectrum
    S_h = (X.t() @ X / n).numpy()
    S = torch.from_numpy(S_h).to(cuda)
    for dtype in (torch.float64, torch.float32):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # a NotConvergedWarning fails the test
            r = de.topk_eigh(S.to(dtype), k)
        assert r.converged
        nblocks = -(-k // 112)
        assert r.sweeps <= 60 * nblocks, f"{dtype}: {r.sweeps} sweeps for {nblocks} blocks"
        V = r.V.double().cpu().numpy()
        ev = r.evals.double().cpu().numpy()
        np.testing.assert_allclose(V.T @ V, np.eye(k), atol=2e-5)
        w, Vr = ref_cpu.top_k_eigh(S_h, k)
        lmax = w[-1]
        assert ref_cpu.projector_distance(V[:, -rank:], Vr[:, -rank:]) <= P_TOL
        np.testing.assert_allclose(ev[-rank:], w[-rank:], rtol=EV_TOL)
        assert np.abs(ev[:k - rank]).max() <= 1e-5 * lmax
        R = S_h @ V - V * ev
        assert np.linalg.norm(R, axis=0).max() <= 1e-4 * lmax


def test_k_above_128_small_genuine_eigenvalues(cuda):
    """k = 300 > 128 whose third block holds only small but genuine eigenvalues,
    5e-6 .. 9e-6 of lambda_max (the deflation-residue band used to take
    every block whose Ritz values were <= 1e-5 |lambda_max| and accept it at a residual
    of ~0.1 relative to its own eigenvalues).  They sit above the band now (32 fp32
    ulps of the scale), so they converge to their own relative tolerance: eigenvalues
    within the north_star 1e-5 and the subspace of the whole top-k at the bar."""
    import distributed_eigenspaces_amd as de
    d, k = 512, 300
    lam = np.concatenate([np.linspace(10.0, 1.0, 224), np.linspace(9e-5, 5e-5, 76),
                          np.linspace(1e-5, 0.0, d - 300)])
    S, S_h = planted(d, lam, seed=13, device=cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = de.topk_eigh(S, k)
    w, Vr = ref_cpu.top_k_eigh(S_h, k)
    ev = r.evals.double().cpu().numpy()
    np.testing.assert_allclose(ev, w, rtol=EV_TOL)
    assert ref_cpu.projector_distance(r.V.double().cpu().numpy()[:, -224:], Vr[:, -224:]) <= P_TOL
