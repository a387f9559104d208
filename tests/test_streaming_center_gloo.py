"""World-size-2 gloo test of StreamingOja(center="running") on CPU: the running centre is the
float64 mean of every row BOTH ranks have seen as of the last aggregation plus this rank's own
rows since, nothing counted twice after a second aggregation, and the ranks' bases agree.  The
Oja step, the server solve and the column sums are CPU stand-ins."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NB, D, K, AGG = 4, 12, 3, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(rank):
    return 48 + 16 * rank  # the ranks' batches differ in size: the pooled mean weighs by rows


def _batches(rank):
    rng = np.random.default_rng(200 + rank)
    scale = np.linspace(3.0, 1.0, D)
    off = np.linspace(-5.0, 7.0, D) * (1 + rank)
    return [(rng.standard_normal((_rows(rank), D)) * scale + off).astype(np.float32) for _ in range(NB)]


def _cpu_oja_step(Xb, V, eta, center=None):
    """CPU stand-in for linalg.oja_step: V <- qr(V + eta/b T^T T V), T = Xb - center."""
    T = Xb.double() if center is None else Xb.double() - center
    v = V.double() + eta * (T.t() @ (T @ V.double())) / Xb.shape[0]
    V.copy_(torch.linalg.qr(v)[0])


def _cpu_server(Wt, k, scale, q0):
    from oracle import ref_cpu
    W = Wt.double().numpy()
    Vs = [W[i * k:(i + 1) * k].T for i in range(W.shape[0] // k)]
    _, v = ref_cpu.top_k_eigh(ref_cpu.projector_average(Vs, 1) * scale, k)
    return torch.from_numpy(v).float()


def _cpu_sums(X):
    return X.double().sum(0)


def _run(rank, world, port, out):
    from distributed_eigenspaces_amd.streaming import StreamingOja
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    V0 = torch.linalg.qr(torch.from_numpy(np.random.default_rng(7).standard_normal((D, K))))[0]
    est = StreamingOja(V0.float(), eta=0.05, agg_every=AGG, step_fn=_cpu_oja_step,
                       server_fn=_cpu_server, sums_fn=_cpu_sums, center="running")
    assert est.mean_ is None
    means = []
    for xb in _batches(rank):
        est.partial_fit(torch.from_numpy(xb))
        means.append(est.mean_.clone())
    assert est.aggregations == NB // AGG
    torch.save((torch.stack(means), est.V.contiguous()), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _mean_of(parts):
    return np.concatenate(parts).astype(np.float64).mean(0)


def test_gloo_world2_running_centre(tmp_path):
    world = 2
    mp.spawn(_run, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(world)]
    data = [_batches(r) for r in range(world)]
    for r in range(world):
        means = got[r][0].numpy()
        o = 1 - r
        for i in range(NB):
            seen_other = (i + 1) // AGG * AGG  # the other rank's rows as of the last aggregation
            want = _mean_of(data[r][:i + 1] + data[o][:seen_other])
            np.testing.assert_allclose(means[i], want, rtol=1e-12, atol=0,
                                       err_msg=f"rank {r} after batch {i}")
    # after each aggregation (batches 2 and 4) both ranks hold the mean of all rows seen by
    # both; the second one would be off if the first pooled sums had been counted again
    for i in (AGG - 1, 2 * AGG - 1):
        want = _mean_of(data[0][:i + 1] + data[1][:i + 1])
        for r in range(world):
            np.testing.assert_allclose(got[r][0][i].numpy(), want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[0][0][i].numpy(), got[1][0][i].numpy(), rtol=1e-12, atol=0)
    assert torch.equal(got[0][1], got[1][1])  # every rank adopted the broadcast basis
    assert torch.isfinite(got[0][1]).all()
