"""Model use of a basis: the fused centred transform vs ``project`` vs the torch composition.

At n x d samples (2^20 x 3072 by default) and each k, three ways are timed with HIP events
in this one process, alternating so that a clock or neighbour effect hits all of them:

* ``linalg.project(X, W)``: Y = X W only (no centring, no norms) - the existing call;
* ``linalg.pca_transform(X, W, mean, residual=True, energy=True)``: Y = (X - mean) W, the
  row energies and the reconstruction errors from one pass over X;
* the torch composition that gives the same three outputs without the kernel:
  T = X - mean (an n x d temporary), Y = T W, energy = sum T^2, resid = energy - sum Y^2.

Rates are the algorithm's own counts over the call time (W pack included): 4 n d bytes of
X against 8 TB/s, 2 n d kp flops (kp = k rounded up to 16, what the MFMAs issue) against
the 155 TF measured fp32-MFMA peak.  They are whole-call figures, not kernel shares.

Prints one JSON line and writes it to --out (committed as profiles/pca_transform.json).

    python tools/pca_transform_bench.py [--n 1048576] [--d 3072] [--ks 16,64] [--steps 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_eigenspaces_amd import linalg  # noqa: E402

HBM_BYTES_PER_S = 8e12
FP32_MFMA_FLOPS = 155e12


def time_events(fn, reps, stream):
    """Mean ms of fn() over reps calls, HIP events on ``stream`` (bench.py's time_events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run_k(X, mean, k, steps, warmup, dev):
    n, d = X.shape
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    W = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0].float().to(dev)
    W = W.t().contiguous().t()  # column-major, as the solvers return it
    mean32 = mean.to(torch.float32)
    st = torch.cuda.current_stream(dev)

    def project():
        return linalg.project(X, W)

    def fused():
        return linalg.pca_transform(X, W, mean, residual=True, energy=True)

    def composed():
        T = X - mean32
        Y = T @ W
        en = (T * T).sum(dim=1)
        return Y, (en - (Y * Y).sum(dim=1)).clamp_min_(0), en

    ways = {"project": project, "fused": fused, "torch": composed}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    torch.cuda.synchronize()
    trials = {name: [] for name in ways}
    for _ in range(3):
        for name, fn in ways.items():
            trials[name].append(time_events(fn, steps, st))
    Yf, rf, ef = fused()
    Yt, rt, et = composed()
    torch.cuda.synchronize()
    kp = (k + 15) // 16 * 16
    out = {"k": k, "kp": kp}
    for name in ways:
        ms = min(trials[name])
        out[f"{name}_ms"] = ms
        out[f"{name}_ms_trials"] = trials[name]
        out[f"{name}_frac_hbm"] = 4.0 * n * d / (ms * 1e-3) / HBM_BYTES_PER_S
    for name in ("project", "fused"):
        out[f"{name}_frac_fp32_mfma"] = 2.0 * n * d * kp / (out[f"{name}_ms"] * 1e-3) / FP32_MFMA_FLOPS
    out["fused_over_project"] = out["fused_ms"] / out["project_ms"]
    out["torch_over_fused"] = out["torch_ms"] / out["fused_ms"]
    # the two ways agree (fp32 sums in different orders; the composition rounds the mean to fp32)
    out["max_abs_dY_fused_vs_torch"] = float((Yf - Yt).abs().max())
    out["max_rel_denergy_fused_vs_torch"] = float(((ef - et).abs() / et).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=3072)
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_transform.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_transform_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn((a.n, a.d), generator=g, device=dev, dtype=torch.float32)
    X += 100.0  # a mean 100x the spread
    mean = linalg.column_sums(X) / a.n
    res = {"tool": "pca_transform_bench", "device": torch.cuda.get_device_name(0), "n": a.n,
           "d": a.d, "steps": a.steps, "warmup": a.warmup,
           "timing": "HIP events around whole calls, best of 3 means, the three ways alternated",
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "fp32_mfma_flops": FP32_MFMA_FLOPS},
           "ks": {}}
    for k in (int(s) for s in a.ks.split(",")):
        res["ks"][str(k)] = run_k(X, mean, k, a.steps, a.warmup, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
