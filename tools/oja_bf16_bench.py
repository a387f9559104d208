"""Oja steps on bf16 samples taken as they are, against widening them first.

At each shape three routes over the same bf16 samples are timed with HIP events in this one
process, alternating so that a clock or neighbour effect hits all of them:

* (a) ``linalg.oja_steps(x_bf16, algo="two_pass")``: the bf16 kernels (csrc/oja.hip, the
  two-pass kernels on the sample type: two MFMAs per fragment pair, X read at 2 bytes);
* (b) ``linalg.oja_steps(x_bf16.float(), algo="two_pass")``: what a bf16 stream cost before
  on a shape the resident kernel cannot take - the widening (an n x d float32 temporary)
  timed with the float32 two-pass kernels;
* (c) ``linalg.oja_steps(x_bf16.float(), algo="auto")``: the same with the library's choice,
  the resident kernel at config 4's shape (at the other shape it is (b) again).

Every call is one run over all the batches; the figures are per batch.  Each route is timed
``--trials`` times (``--steps`` calls a trial) after ``--warmup`` calls; the median and the
spread (min, max) of the trials are reported, at the clocks as found.  (a) and (b) must
return the same bits, which the run checks.

Prints one JSON line and writes it to --out (committed as profiles/oja_bf16.json).

    python tools/oja_bf16_bench.py [--shapes 4096x3072x32x64x8,4096x8192x64x16x8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_eigenspaces_amd import linalg  # noqa: E402

ETA = 0.02


def time_events(fn, reps, stream):
    """Mean ms of fn() over reps calls, HIP events on ``stream`` (bench.py's time_events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(ways, steps, warmup, trials, stream):
    """{name: [ms of each trial]}: warm every way, then ``trials`` rounds over all of them."""
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in ways}
    for _ in range(trials):
        for name, fn in ways.items():
            out[name].append(time_events(fn, steps, stream))
    return out


def make_samples(n, d, dev):
    """(n, d) bf16 samples randn, generated in row blocks (no n x d float32 temporary)."""
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    step = max(1, (1 << 26) // d)
    for lo in range(0, n, step):
        blk = torch.randn((min(step, n - lo), d), generator=g, device=dev, dtype=torch.float32)
        x[lo:lo + blk.shape[0]] = blk.to(torch.bfloat16)
    return x


def run_shape(b, d, k, nb, orth, steps, warmup, trials, dev):
    x = make_samples(nb * b, d, dev)
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    V0 = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0].float().to(dev)
    # a column-major buffer each (V0 is column-major already: V0.t().contiguous() would be V0 itself)
    Vs = {name: torch.empty((k, d), dtype=torch.float32, device=dev).t() for name in ("a", "b", "c")}

    def route(name, widen, algo):
        def fn():
            Vs[name].copy_(V0)
            linalg.oja_steps(x.float() if widen else x, Vs[name], ETA, b, orth, algo=algo, check=False)
        return fn
    ways = {"a_bf16": route("a", False, "two_pass"),
            "b_widen_two_pass": route("b", True, "two_pass"),
            "c_widen_auto": route("c", True, "auto")}
    res = interleaved(ways, steps, warmup, trials, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    linalg.oja_check(dev, b, d, k)  # route (c)'s resident hand-offs: none timed out
    out = {"b": b, "d": d, "k": k, "batches": nb, "orth_every": orth,
           "c_is_resident": bool(b == 4096 and d % 512 == 0 and d <= 3072 and k <= 32)}
    for name in ways:
        per_batch = [t / nb for t in res[name]]
        out[f"{name}_ms_per_batch"] = statistics.median(per_batch)
        out[f"{name}_ms_per_batch_min_max"] = [min(per_batch), max(per_batch)]
        out[f"{name}_ms_per_batch_trials"] = per_batch
    out["a_over_b"] = out["a_bf16_ms_per_batch"] / out["b_widen_two_pass_ms_per_batch"]
    out["a_over_c"] = out["a_bf16_ms_per_batch"] / out["c_widen_auto_ms_per_batch"]
    # (c) beats (a) by more than the run-to-run spread: every trial of (c) below every one of (a)
    out["c_faster_than_a_beyond_spread"] = (out["c_widen_auto_ms_per_batch_min_max"][1]
                                            < out["a_bf16_ms_per_batch_min_max"][0])
    out["a_faster_than_c_beyond_spread"] = (out["a_bf16_ms_per_batch_min_max"][1]
                                            < out["c_widen_auto_ms_per_batch_min_max"][0])
    out["a_bits_equal_b"] = bool(torch.equal(Vs["a"], Vs["b"]))
    out["a_finite"] = bool(torch.isfinite(Vs["a"]).all())
    # bytes of X a batch reads: (a) twice 2 B; (b) the widening (2 + 4) and twice 4 B
    out["a_x_bytes_per_batch"] = 2 * 2 * b * d
    out["b_x_bytes_per_batch"] = (2 + 4 + 2 * 4) * b * d
    out["a_frac_hbm"] = out["a_x_bytes_per_batch"] / (out["a_bf16_ms_per_batch"] * 1e-3) / 8e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x3072x32x64x8,4096x8192x64x16x8",
                    help="comma list of b x d x k x batches x orth_every")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oja_bf16.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("oja_bf16_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    res = {"tool": "oja_bf16_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "trials": a.trials,
           "timing": "HIP events around whole calls (all batches, both re-orthonormalisations "
                     "included), per batch; median and min/max of the trials, the routes "
                     "alternated, clocks as found",
           "shapes": []}
    for shape in a.shapes.split(","):
        b, d, k, nb, orth = (int(v) for v in shape.split("x"))
        res["shapes"].append(run_shape(b, d, k, nb, orth, a.steps, a.warmup, a.trials, dev))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
