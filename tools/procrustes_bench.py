"""Server-side aggregation: Procrustes average vs the projector-average top-k solve.

For each server shape the same synthetic stack of m worker bases
(V_i = qr(U + eps / sqrt(d) N_i) Q_i around a planted U) goes through
``linalg.procrustes_average`` and through ``linalg.projavg_topk`` warm-started from
V_1 as the estimator's server does; both are timed with HIP events in this one
process, and both results' distance to the planted subspace is recorded.  The
per-kernel split of the Procrustes pass comes from the kernel durations the torch
profiler records for a few extra calls (stages told apart by the fixed launch order),
with two event-timed stand-ins beside it: the stack-sized products run alone through
``linalg.gemm_skinny`` (the same kernel, the same shapes).

Prints one JSON line (committed as profiles/procrustes_server.json).

    python tools/procrustes_bench.py [--shapes c3,c4agg,c5] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_eigenspaces_amd import linalg  # noqa: E402
from oracle import ref_cpu  # noqa: E402

SHAPES = {  # name: (m, k, d)
    "c3": (8, 64, 8192),
    "c5": (64, 128, 16384),
    "c4agg": (8, 32, 3072),
}


def time_events(fn, reps, stream):
    """Mean ms of fn() over reps calls, HIP events on ``stream`` (bench.py's time_events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def synthetic_stack(m, k, d, eps, seed, dev):
    """Wt ((m k) x d, fp32 on dev) and the planted U (float64, host)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    U = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0]
    rows = []
    for _ in range(m):
        N = torch.randn(d, k, generator=g, dtype=torch.float64)
        Q = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64))[0]
        V = torch.linalg.qr(U + (eps / d ** 0.5) * N)[0] @ Q
        rows.append(V.t().to(torch.float32))
    return torch.cat(rows, dim=0).contiguous().to(dev), U.numpy()


STAGES = ("cross_gram", "polar", "combine", "loewdin")


def kernel_split(fn, calls):
    """Mean ms per call of each stage from the profiler's kernel durations.  Launch order
    of one pass: weights, reference image, product 1 (+ reduce) | small SVD (m groups) |
    product 2 (+ reduce) | twice: product, (+ reduce), small SVD, apply."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    evs = []
    for e in prof.events():
        if "cuda" not in str(getattr(e, "device_type", "")).lower():
            continue
        dur = getattr(e, "device_time", None)
        if dur is None:
            dur = getattr(e, "cuda_time", 0.0)
        evs.append((e.time_range.start, e.name, float(dur)))
    evs.sort()
    tot = dict.fromkeys(STAGES, 0.0)
    nprod, seen = 0, 0
    for _, name, us in evs:
        if "fill_kernel" in name or "set_weights_kernel" in name:
            nprod = 0
            seen += 1
            tot["cross_gram"] += us
        elif "skinny_reduce_kernel" in name or "ref_rows_kernel" in name:
            tot["cross_gram" if nprod <= 1 else "combine" if nprod == 2 else "loewdin"] += us
        elif "skinny_kernel" in name:
            nprod += 1
            tot["cross_gram" if nprod == 1 else "combine" if nprod == 2 else "loewdin"] += us
        elif "small_svd_kernel" in name:
            tot["polar" if nprod == 1 else "loewdin"] += us
        elif "apply_kernel" in name:
            tot["loewdin"] += us
    if seen != calls:
        raise RuntimeError(f"profiler saw {seen} passes, expected {calls}")
    return {s: tot[s] / calls / 1e3 for s in STAGES}


def run_shape(name, steps, warmup, eps, dev):
    m, k, d = SHAPES[name]
    Wt, U = synthetic_stack(m, k, d, eps, 1234, dev)
    st = torch.cuda.current_stream(dev)
    q0 = Wt[:k].t()

    def proc():
        return linalg.procrustes_average(Wt, k)

    def proj():
        return linalg.projavg_topk(Wt, k, 1.0 / m, q0=q0)

    for _ in range(warmup):
        proc()
        proj()
    torch.cuda.synchronize()
    # alternate the two so that a clock or neighbour effect hits both
    t_proc, t_proj = [], []
    for _ in range(3):
        t_proc.append(time_events(proc, steps, st))
        t_proj.append(time_events(proj, steps, st))
    pr, pj = proc(), proj()
    torch.cuda.synchronize()
    out = {
        "m": m, "k": k, "d": d, "eps": eps,
        "procrustes_ms": min(t_proc), "procrustes_ms_trials": t_proc,
        "projavg_ms": min(t_proj), "projavg_ms_trials": t_proj,
        "projavg_sweeps": pj.sweeps, "projavg_converged": bool(pj.converged),
        "speedup": min(t_proj) / min(t_proc),
        "dist_planted_procrustes": ref_cpu.projector_distance(pr.V.cpu().numpy(), U),
        "dist_planted_projavg": ref_cpu.projector_distance(pj.V.cpu().numpy(), U),
        "dist_planted_worker1": ref_cpu.projector_distance(Wt[:k].t().cpu().numpy(), U),
        "dist_procrustes_projavg_device": linalg.projector_distance(pr.V, pj.V),
        "min_cosine": float(pr.cosines.min()),
    }
    # the two stack-sized products alone (same kernel and shapes as inside the pass)
    kp = (k + 15) // 16 * 16
    R = torch.zeros((d, kp), dtype=torch.float32, device=dev)
    R[:, :k] = Wt[:k].t()
    G = torch.empty((m * k, kp), dtype=torch.float32, device=dev)
    Vb = torch.empty((d, kp), dtype=torch.float32, device=dev)
    linalg.gemm_skinny(Wt, R, False, C=G)
    linalg.gemm_skinny(Wt, G, True, C=Vb)
    out["product_wt_r_ms"] = time_events(lambda: linalg.gemm_skinny(Wt, R, False, C=G), steps, st)
    out["product_wtT_z_ms"] = time_events(lambda: linalg.gemm_skinny(Wt, G, True, C=Vb), steps, st)
    flops = 2 * 2.0 * m * k * d * kp
    out["stack_products_tflops"] = flops / ((out["product_wt_r_ms"] + out["product_wtT_z_ms"]) * 1e9)
    try:
        out["kernel_split_ms"] = kernel_split(proc, 5)
    except Exception as e:  # noqa: BLE001 - the split is a by-product; say why it is missing
        out["kernel_split_ms"] = None
        out["kernel_split_error"] = f"{type(e).__name__}: {e}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4agg,c3,c5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("procrustes_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    res = {"tool": "procrustes_bench", "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "warmup": a.warmup, "timing": "HIP events, best of 3 means",
           "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = run_shape(name, a.steps, a.warmup, a.eps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
