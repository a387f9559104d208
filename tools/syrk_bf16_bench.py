"""Covariance and transform of bf16 samples taken as they are, against widening them first.

At each shape three ways to the covariance of the same bf16 samples are timed with HIP events
in this one process, alternating so that a clock or neighbour effect hits all of them:

* (a) ``linalg.sigma_hat(x_bf16)``: the bf16 kernel (csrc/syrk_bf16.hip), image pass,
  SYRK and reduction included;
* (b) ``linalg.sigma_hat(x_bf16.float())``: what a bf16 shard cost before - the widening
  (an n x d float32 temporary) and the split3 SYRK of the copy;
* (c) ``linalg.sigma_hat(x_f32, algo="split3")`` on an already widened copy: kernel against
  kernel.

The fraction of the bf16 peak counts the algorithm's own flops, n d (d + 1) (the lower
triangle, multiply and add), against 2.5 PF.  The same run times the fused transform of the
bf16 samples against ``pca_transform(x.float())`` (widening included) at --tn x --td.

Prints one JSON line and writes it to --out (committed as profiles/syrk_bf16.json).

    python tools/syrk_bf16_bench.py [--shapes 524288x8192,1048576x3072] [--steps 5]
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

BF16_MFMA_FLOPS = 2.5e15


def time_events(fn, reps, stream):
    """Mean ms of fn() over reps calls, HIP events on ``stream`` (bench.py's time_events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(ways, steps, warmup, stream):
    """{name: [ms of 3 trials]}: warm every way, then 3 rounds over all of them."""
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    torch.cuda.synchronize()
    trials = {name: [] for name in ways}
    for _ in range(3):
        for name, fn in ways.items():
            trials[name].append(time_events(fn, steps, stream))
    return trials


def make_samples(n, d, dev):
    """(n, d) bf16 samples 3 randn + 1, generated in row blocks (no n x d float32 temporary)."""
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    step = max(1, (1 << 26) // d)
    for lo in range(0, n, step):
        blk = torch.randn((min(step, n - lo), d), generator=g, device=dev, dtype=torch.float32)
        x[lo:lo + blk.shape[0]] = (3.0 * blk + 1.0).to(torch.bfloat16)
    return x


def run_syrk(n, d, steps, warmup, dev):
    x = make_samples(n, d, dev)
    xf = x.float()
    S = torch.empty((d, d), dtype=torch.float32, device=dev)
    Sf = torch.empty((d, d), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)
    ways = {"a_bf16": lambda: linalg.sigma_hat(x, out=S),
            "b_widen_split3": lambda: linalg.sigma_hat(x.float(), out=Sf, algo="split3"),
            "c_split3": lambda: linalg.sigma_hat(xf, out=Sf, algo="split3")}
    trials = interleaved(ways, steps, warmup, st)
    ways["a_bf16"]()
    ways["c_split3"]()
    torch.cuda.synchronize()
    out = {"n": n, "d": d}
    for name in ways:
        out[f"{name}_ms"] = min(trials[name])
        out[f"{name}_ms_trials"] = trials[name]
    flops = float(n) * d * (d + 1)
    out["a_frac_bf16_peak"] = flops / (out["a_bf16_ms"] * 1e-3) / BF16_MFMA_FLOPS
    out["c_frac_bf16_peak_useful"] = flops / (out["c_split3_ms"] * 1e-3) / BF16_MFMA_FLOPS
    out["a_over_b"] = out["a_bf16_ms"] / out["b_widen_split3_ms"]
    out["a_over_c"] = out["a_bf16_ms"] / out["c_split3_ms"]
    out["a_faster_than_c_by_more_than_3_percent"] = out["a_over_c"] < 1.0 / 1.03
    out["max_abs_dS_over_max_S"] = float((S - Sf).abs().max() / Sf.abs().max())
    nb = linalg._lib.lib()
    out["a_workspace_bytes"] = int(nb.deig_syrk_bf16_workspace(n, d))
    out["c_workspace_bytes"] = int(nb.deig_syrk_workspace_ex(n, d, linalg._lib.DEIG_SYRK_SPLIT3))
    return out


def run_transform(n, d, k, steps, warmup, dev, x):
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    W = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0].float().to(dev)
    W = W.t().contiguous().t()  # column-major, as the solvers return it
    mean = linalg.column_sums(x) / n
    st = torch.cuda.current_stream(dev)
    ways = {"bf16": lambda: linalg.pca_transform(x, W, mean, residual=True, energy=True),
            "widen_f32": lambda: linalg.pca_transform(x.float(), W, mean, residual=True, energy=True)}
    trials = interleaved(ways, steps, warmup, st)
    Yb = ways["bf16"]()[0]
    Yf = ways["widen_f32"]()[0]
    torch.cuda.synchronize()
    out = {"k": k}
    for name in ways:
        out[f"{name}_ms"] = min(trials[name])
        out[f"{name}_ms_trials"] = trials[name]
    out["bf16_over_widen_f32"] = out["bf16_ms"] / out["widen_f32_ms"]
    out["bf16_frac_hbm"] = 2.0 * n * d / (out["bf16_ms"] * 1e-3) / 8e12
    out["max_abs_dY"] = float((Yb - Yf).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="524288x8192,1048576x3072")
    ap.add_argument("--tn", type=int, default=1 << 20)
    ap.add_argument("--td", type=int, default=3072)
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syrk_bf16.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("syrk_bf16_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    res = {"tool": "syrk_bf16_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup,
           "timing": "HIP events around whole calls, best of 3 means, the ways alternated",
           "peaks": {"bf16_mfma_flops": BF16_MFMA_FLOPS}, "syrk": [], "transform": {}}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        res["syrk"].append(run_syrk(n, d, a.steps, a.warmup, dev))
        torch.cuda.empty_cache()
    if a.ks:
        x = make_samples(a.tn, a.td, dev)
        res["transform"] = {"n": a.tn, "d": a.td, "ks": {}}
        for k in (int(s) for s in a.ks.split(",")):
            res["transform"]["ks"][str(k)] = run_transform(a.tn, a.td, k, a.steps, a.warmup, dev, x)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
