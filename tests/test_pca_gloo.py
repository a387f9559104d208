"""World-size-2 gloo tests of the centred fit's host logic on CPU: the pooled mean
(one all-reduce of [column sums, row count]) and its hand-over to every logical worker.
The per-worker GPU compute is replaced by a fake that records what it was given."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_eigenspaces_amd.estimator import (DistributedEigenspaceEstimator, gather_bases,
                                                   global_mean)

ROWS = (3, 5)  # rank 0, rank 1: unequal on purpose (a mean of means would be wrong)
D = 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(rank):
    # on a 2^-10 grid: every partial sum is exact in double, so any summation order gives
    # the same sums and the pooled mean is one correctly rounded division
    rng = np.random.default_rng(40 + rank)
    x = 1000.0 + rng.standard_normal((ROWS[rank], D)) * np.linspace(1.0, 3.0, D)
    return np.round(x * 1024.0) / 1024.0


def _run_mean(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.from_numpy(_rows(rank))
    mu = global_mean(x.sum(dim=0), x.shape[0])
    torch.save(mu, os.path.join(out, f"mu{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_global_mean(tmp_path):
    mp.spawn(_run_mean, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    m0 = torch.load(os.path.join(tmp_path, "mu0.pt"), weights_only=True)
    m1 = torch.load(os.path.join(tmp_path, "mu1.pt"), weights_only=True)
    assert m0.dtype == torch.float64 and m0.shape == (D,)
    assert torch.equal(m0, m1)  # the same bits on both ranks
    ref = np.concatenate([_rows(0), _rows(1)]).mean(axis=0)
    np.testing.assert_allclose(m0.numpy(), ref, rtol=1e-15)
    # not the mean of the two ranks' means
    wrong = 0.5 * (_rows(0).mean(axis=0) + _rows(1).mean(axis=0))
    assert np.max(np.abs(wrong - ref) / np.abs(ref)) > 1e-9


def test_global_mean_single_process():
    x = torch.from_numpy(_rows(1))
    mu = global_mean(x.sum(dim=0), x.shape[0])
    np.testing.assert_allclose(mu.numpy(), _rows(1).mean(axis=0), rtol=1e-15)


def _recording_worker(x, k, center=None, **kw):
    """Basis rows: the centre this worker received, then its shard's row count."""
    d = x.shape[1]
    V = torch.zeros((d, k), dtype=torch.float64)
    V[:, 0] = center
    V[0, 1] = x.shape[0]
    return V, torch.arange(k, dtype=torch.float32), 1


def _run_fit(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.from_numpy(_rows(rank))
    est = DistributedEigenspaceEstimator(2, workers_per_rank=2, worker_fn=_recording_worker,
                                         center=True)
    mu = est.pooled_mean(x)
    Wt_local, _, _ = est.local_bases(x, mu)
    Wt = gather_bases(Wt_local)
    torch.save({"mu": mu, "Wt": Wt}, os.path.join(out, f"fit{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_fit_hands_the_pooled_mean_to_every_worker(tmp_path):
    mp.spawn(_run_fit, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(os.path.join(tmp_path, "fit0.pt"), weights_only=True)
    r1 = torch.load(os.path.join(tmp_path, "fit1.pt"), weights_only=True)
    assert torch.equal(r0["mu"], r1["mu"]) and torch.equal(r0["Wt"], r1["Wt"])
    # two workers per rank use 2 * (n // 2) rows: 2 of rank 0's 3, 4 of rank 1's 5
    ref = np.concatenate([_rows(0)[:2], _rows(1)[:4]]).mean(axis=0)
    np.testing.assert_allclose(r0["mu"].numpy(), ref, rtol=1e-15)
    Wt = r0["Wt"]
    assert Wt.shape == (2 * 2 * 2, D)
    for w in range(4):  # every logical worker of both ranks got the same centre
        assert torch.equal(Wt[2 * w], r0["mu"]), w
    assert [int(Wt[2 * w + 1, 0]) for w in range(4)] == [1, 1, 2, 2]


def test_uncentred_fit_passes_no_center():
    """The default path is unchanged: an injected worker sees no ``center`` keyword."""
    seen = {}

    def worker(x, k, **kw):
        seen.update(kw)
        return torch.zeros((x.shape[1], k)), torch.zeros(k), 1

    est = DistributedEigenspaceEstimator(2, worker_fn=worker)
    est.local_bases(torch.zeros((4, D)))
    assert "center" not in seen and est.center is False
