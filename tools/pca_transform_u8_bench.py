"""Model use of a basis on uint8 samples: the fused byte transform vs widening first.

Two shapes by default - 2^20 x 3072 raw bytes, and 2^20 x 1024 grey pixels (3072 bytes a row)
- and each k.  Three ways to the same three outputs (scores, row energies, reconstruction
errors) are timed with HIP events in this one process, alternating so that a clock or
neighbour effect hits all of them:

* ``u8``: ``linalg.pca_transform_u8(x, W, mean, mode, residual=True, energy=True)`` - the
  bytes are read once, centred in the kernel;
* ``widen``: today's route with the widening in the timed region - ``x.float()`` (raw) or
  the channel mean of the float pixels (grey), then ``linalg.pca_transform``;
* ``f32``: ``linalg.pca_transform`` alone on floats widened beforehand.

Rates are the algorithm's own byte counts over the call time (W pack included) against
8 TB/s: the bytes of x for ``u8`` (n d raw, 3 n d grey), 4 n d for ``f32``.  They are
whole-call figures, not kernel shares.

Prints one JSON line and writes it to --out (committed as profiles/pca_transform_u8.json).

    python tools/pca_transform_u8_bench.py [--n 1048576] [--ks 16,64] [--steps 20]
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


def time_events(fn, reps, stream):
    """Mean ms of fn() over reps calls, HIP events on ``stream`` (bench.py's time_events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def widen(x, mode, d):
    """Today's widening: the floats ``pca_transform`` reads."""
    if mode == "raw":
        return x.float()
    return x.view(x.shape[0], d, 3).float().mean(dim=2)


def run_k(x, xf, mode, d, mean, k, steps, warmup, dev):
    n = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    W = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0].float().to(dev)
    W = W.t().contiguous().t()  # column-major, as the solvers return it
    st = torch.cuda.current_stream(dev)

    def u8():
        return linalg.pca_transform_u8(x, W, mean, mode, residual=True, energy=True)

    def widened():
        return linalg.pca_transform(widen(x, mode, d), W, mean, residual=True, energy=True)

    def f32():
        return linalg.pca_transform(xf, W, mean, residual=True, energy=True)

    ways = {"u8": u8, "widen": widened, "f32": f32}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    torch.cuda.synchronize()
    trials = {name: [] for name in ways}
    for _ in range(3):
        for name, fn in ways.items():
            trials[name].append(time_events(fn, steps, st))
    Yu, ru, eu = u8()
    Yf, rf, ef = f32()
    torch.cuda.synchronize()
    out = {"k": k, "kp": (k + 15) // 16 * 16}
    for name in ways:
        out[f"{name}_ms"] = min(trials[name])
        out[f"{name}_ms_trials"] = trials[name]
    bytes_u8 = float(n) * d * (1 if mode == "raw" else 3)
    out["u8_frac_hbm"] = bytes_u8 / (out["u8_ms"] * 1e-3) / HBM_BYTES_PER_S
    out["f32_frac_hbm"] = 4.0 * n * d / (out["f32_ms"] * 1e-3) / HBM_BYTES_PER_S
    out["widen_over_u8"] = out["widen_ms"] / out["u8_ms"]
    out["f32_over_u8"] = out["f32_ms"] / out["u8_ms"]
    # the ways agree (fp32 sums in different orders; grey floats are rounded before centring)
    out["max_abs_dY_u8_vs_f32"] = float((Yu - Yf).abs().max())
    out["max_rel_denergy_u8_vs_f32"] = float(((eu - ef).abs() / ef).max())
    return out


def run_shape(mode, n, d, ks, steps, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(7 if mode == "raw" else 8)
    width = d if mode == "raw" else 3 * d
    # bytes around 128 with a spread of 30: a mean several times the spread, as images have
    x = (128.0 + 30.0 * torch.randn((n, width), generator=g, device=dev)).clamp_(0, 255).to(torch.uint8)
    mean = linalg.column_sums_u8(x, mode) / n
    xf = widen(x, mode, d)
    res = {"mode": mode, "n": n, "d": d, "row_bytes": width, "ks": {}}
    for k in ks:
        res["ks"][str(k)] = run_k(x, xf, mode, d, mean, k, steps, warmup, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d-raw", type=int, default=3072)
    ap.add_argument("--d-gray", type=int, default=1024)
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_transform_u8.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_transform_u8_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    ks = [int(s) for s in a.ks.split(",")]
    res = {"tool": "pca_transform_u8_bench", "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "warmup": a.warmup,
           "timing": "HIP events around whole calls, best of 3 means, the three ways alternated",
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S}, "shapes": []}
    for mode, d in (("raw", a.d_raw), ("gray", a.d_gray)):
        res["shapes"].append(run_shape(mode, a.n, d, ks, a.steps, a.warmup, dev))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
