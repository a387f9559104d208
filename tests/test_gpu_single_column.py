"""Single-column inputs (rank = 1: the top principal component).  torch reports strides
(1, 1) for a (d, 1) tensor whatever its layout, so a leading dimension taken from
``stride(1)`` is 1 and fails the library's ``ld >= d`` rule; every op that takes a basis
or a warm start is run here with one column, against the float64 oracle at the suite's
bars (||P - P_ref||_F <= 1e-4, eigenvalues <= 1e-5 relative)."""
import json

import numpy as np
import pytest
import torch

from distributed_eigenspaces_amd import linalg
from oracle import ref_cpu
from tests.conftest import load_golden
from tests.test_gpu_skinny import project_ratio

pytestmark = pytest.mark.gpu
P_TOL, EV_TOL = 1e-4, 1e-5
NAME = "spiked_d64_k4_m8"


@pytest.mark.parametrize("form", ["1-D", "column"])
def test_topk_eigh_warm_start(form, cuda):
    S32 = load_golden(NAME)["sigma_hat0"].astype(np.float32)
    d = S32.shape[0]
    w, v = ref_cpu.top_k_eigh(S32.astype(np.float64), 1)
    q = v[:, 0] + 0.3 * np.random.default_rng(0).standard_normal(d)  # a rough start
    q = (q / np.linalg.norm(q)).astype(np.float32)
    q0 = torch.from_numpy(q if form == "1-D" else q[:, None]).to(cuda)
    if form == "column":
        assert q0.shape == (d, 1) and q0.is_contiguous()
    r = linalg.topk_eigh(torch.from_numpy(S32).to(cuda), 1, q0=q0)
    assert r.converged and tuple(r.V.shape) == (d, 1)
    assert ref_cpu.projector_distance(r.V.cpu().numpy(), v) <= P_TOL
    np.testing.assert_allclose(r.evals.cpu().numpy(), w, rtol=EV_TOL, atol=0)


def test_projavg_topk_warm_start(cuda):
    """The bases as MasterNode.callback_ makes them: (d, 1) arrays from nested lists."""
    g = load_golden(NAME)
    m = int(g["m"])
    vs = [np.array(g["worker_V"][i][:, -1:].astype(np.float32).tolist()) for i in range(m)]
    assert vs[0].shape == (64, 1)
    bases = [linalg.require_device_tensor(v, "eigenspace") for v in vs]
    r = linalg.projavg_topk(linalg.stack_bases(bases), 1, 1.0 / m, q0=bases[0])
    w, v = ref_cpu.top_k_eigh(ref_cpu.projector_average(vs, m), 1)
    assert r.converged and tuple(r.V.shape) == (64, 1)
    assert ref_cpu.projector_distance(r.V.cpu().numpy(), v) <= P_TOL
    np.testing.assert_allclose(r.evals.cpu().numpy(), w, rtol=EV_TOL, atol=0)


def test_protocol_rank_one(cuda):
    """SlaveNode + MasterNode over the in-process broker with rank = 1."""
    from distributed_eigenspaces_amd import broker as br
    from distributed_eigenspaces_amd import distributed as dd
    g = load_golden(NAME)
    X, m = g["X"], int(g["m"])
    b = br.InProcBroker("gpu-rank-one")
    dd.SlaveNode(b, X)
    master = dd.MasterNode(b, 1, m, X)
    master.start()
    resps = [json.loads(body) for q, body in b.delivered if q == "master"]
    assert len(resps) == m and np.array(resps[0]["eigenspace"]).shape == (64, 1)
    _, _, sw, sv = ref_cpu.one_shot(X, 1, m)
    assert master.eigenspace.shape == (64, 1)
    assert ref_cpu.projector_distance(master.eigenspace, sv) <= P_TOL
    np.testing.assert_allclose(master.eigenvalues, sw, rtol=EV_TOL)


@pytest.mark.parametrize("order", ["C", "F"])
def test_project_single_column(order, cuda):
    from distributed_eigenspaces_amd import notebook as nb
    rng = np.random.default_rng(3)
    x = rng.standard_normal((130, 64)).astype(np.float32)
    w = np.require(rng.standard_normal((64, 1)).astype(np.float32), requirements=order)
    Y = linalg.project(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda))
    assert tuple(Y.shape) == (130, 1)
    assert project_ratio(Y.cpu().numpy(), x, w) <= 1.0
    y = nb.project(x, w)
    assert isinstance(y, np.ndarray) and y.shape == (130, 1)
    assert project_ratio(y, x, w) <= 1.0


def oja_inputs(cuda):
    from distributed_eigenspaces_amd import synthetic
    d, b, nb = 64, 256, 4
    U = synthetic.planted_basis(d, 1, seed=3, device=cuda)
    X = synthetic.spiked_samples(nb * b, U, seed=4)
    V0 = torch.linalg.qr(torch.randn(d, 1, device=cuda, dtype=torch.float64))[0]
    return X, V0, b, nb


def oja_basis(V0, how):
    """V0 as the (d, 1) float32 tensor oja_step takes: built as the other Oja tests build
    theirs, or freshly allocated - then its strides are (1, 1)."""
    if how == "transposed":
        return V0.float().t().contiguous().t()
    V = torch.empty((V0.shape[0], 1), dtype=torch.float32, device=V0.device).copy_(V0)
    assert V.stride() == (1, 1)
    return V


def check_oja(V, X, V0, eta, b):
    Vg = V.cpu().numpy()
    assert Vg.shape == (64, 1) and np.isfinite(Vg).all()
    np.testing.assert_allclose(Vg.T @ Vg, np.eye(1), atol=1e-5)
    Vr = ref_cpu.oja_epoch(X.double().cpu().numpy(), V0.cpu().numpy(), eta, b)
    assert ref_cpu.projector_distance(Vg, Vr) <= P_TOL


@pytest.mark.parametrize("how", ["transposed", "fresh"])
def test_oja_step_single_column(how, cuda):
    X, V0, b, nb = oja_inputs(cuda)
    V = oja_basis(V0, how)
    for i in range(nb):
        assert linalg.oja_step(X[i * b:(i + 1) * b], V, 0.5) is V
    check_oja(V, X, V0, 0.5, b)


@pytest.mark.parametrize("how", ["transposed", "fresh"])
@pytest.mark.parametrize("orth_every", [1, 3])
def test_oja_steps_single_column(orth_every, how, cuda):
    X, V0, b, _ = oja_inputs(cuda)
    V = oja_basis(V0, how)
    assert linalg.oja_steps(X, V, 0.5, b, orth_every=orth_every) is V
    check_oja(V, X, V0, 0.5, b)


def test_procrustes_and_distance_single_column(cuda):
    """k = 1 with a tensor reference: V = normalise(sum_i sign(v_i . r) v_i / m)."""
    rng = np.random.default_rng(4)
    d, m = 64, 5
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    vs = []
    for i in range(m):
        v = u + 0.3 / np.sqrt(d) * rng.standard_normal(d)
        vs.append(((-1) ** i * v / np.linalg.norm(v)).astype(np.float32)[:, None])
    u32 = u.astype(np.float32)[:, None]
    vbar = sum(np.sign(v.astype(np.float64).T @ u32) * v.astype(np.float64) for v in vs) / m
    ref = vbar / np.linalg.norm(vbar)
    Wt = linalg.stack_bases([torch.from_numpy(v).to(cuda) for v in vs])
    r = linalg.procrustes_average(Wt, 1, ref=torch.from_numpy(u32).to(cuda))
    V = r.V.cpu().numpy().astype(np.float64)
    assert V.shape == (d, 1)
    assert np.linalg.norm(V - ref) <= P_TOL  # the sign follows the reference, too
    assert abs(float(V[:, 0] @ V[:, 0]) - 1.0) <= 1e-5
    cos = np.array([abs(float(v[:, 0].astype(np.float64) @ u32[:, 0])) for v in vs])
    np.testing.assert_allclose(r.cosines.cpu().numpy()[:, 0], cos, atol=EV_TOL)
    # sin of the angle between two unit vectors, from the residual b - a (a . b)
    a, bb = vs[0].astype(np.float64), vs[1].astype(np.float64)
    a, bb = a / np.linalg.norm(a), bb / np.linalg.norm(bb)
    sin = np.linalg.norm(bb - a * float(a[:, 0] @ bb[:, 0]))
    fro, two = linalg.subspace_distance(torch.from_numpy(vs[0]).to(cuda),
                                        torch.from_numpy(vs[1]).to(cuda))
    assert abs(fro - sin) <= 1e-5 and abs(two - sin) <= 1e-5
    assert abs(linalg.projector_distance(torch.from_numpy(vs[0]).to(cuda),
                                         torch.from_numpy(vs[1]).to(cuda))
               - ref_cpu.projector_distance(vs[0], vs[1])) <= 1e-5
