"""Oja steps about a centre on samples taken as they are, against materialising the centred
float32 tensor first; and uint8 samples read as bytes against widening them.

At each shape, for each of float32, bfloat16 and uint8 samples, two routes are timed with HIP
events in this one process, alternating so that a clock or neighbour effect hits all of them:

* (a) ``linalg.oja_steps(x, ..., center=c)``: the centred two-pass kernels (csrc/oja.hip:
  the sample centred where it is staged, fl32((double)x - c), three MFMAs per fragment pair);
* (b) ``linalg.oja_steps((x.double() - c).float(), ..., algo="two_pass")``: what a centred
  stream cost before - the centred n x d float32 tensor (through an n x d float64 temporary)
  timed with the float32 two-pass kernels.

And for uint8 samples without a centre:

* (u8_bytes) ``linalg.oja_steps(x_u8, algo="two_pass")``: the bytes in place (two MFMAs per
  fragment pair, X read at 1 byte);
* (u8_widen_auto) ``linalg.oja_steps(x_u8.float(), algo="auto")``: widening plus the library's
  choice, the resident kernel at config 4's shape.

Every call is one run over all the batches; the figures are per batch.  Each route is timed
``--trials`` times (``--steps`` calls a trial) after ``--warmup`` calls; the median and the
spread (min, max) of the trials are reported, at the clocks as found.  (a) and (b) must return
the same bits, which the run checks (it exits non-zero otherwise).

Prints one JSON line and writes it to --out (committed as profiles/oja_centered.json).

    python tools/oja_centered_bench.py [--shapes 4096x3072x32x64x8,4096x8192x64x16x8]
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
from tools.oja_bf16_bench import interleaved  # noqa: E402

ETAS = {"f32": 0.02, "bf16": 0.02, "u8": 0.02 / 24.0 ** 2}
ELEM_BYTES = {"f32": 4, "bf16": 2, "u8": 1}


def make_samples(n, d, dev):
    """{kind: (n, d) samples} from one randn stream generated in row blocks: float32 as it is,
    bfloat16 with a mean of 3, bytes clip(rint(128 + 24 x))."""
    g = torch.Generator(device=dev).manual_seed(7)
    xs = {"f32": torch.empty((n, d), dtype=torch.float32, device=dev),
          "bf16": torch.empty((n, d), dtype=torch.bfloat16, device=dev),
          "u8": torch.empty((n, d), dtype=torch.uint8, device=dev)}
    step = max(1, (1 << 26) // d)
    for lo in range(0, n, step):
        blk = torch.randn((min(step, n - lo), d), generator=g, device=dev, dtype=torch.float32)
        hi = lo + blk.shape[0]
        xs["f32"][lo:hi] = blk
        xs["bf16"][lo:hi] = (blk + 3).to(torch.bfloat16)
        xs["u8"][lo:hi] = torch.clip(torch.round(128 + 24 * blk), 0, 255).to(torch.uint8)
    return xs


def column_mean(x):
    if x.dtype == torch.uint8:
        return linalg.column_sums_u8(x, "raw") / x.shape[0]
    return linalg.column_sums(x) / x.shape[0]


def run_shape(b, d, k, nb, orth, steps, warmup, trials, dev):
    xs = make_samples(nb * b, d, dev)
    cs = {kind: column_mean(x) for kind, x in xs.items()}
    g = torch.Generator(device="cpu").manual_seed(100 + k)
    V0 = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0].float().to(dev)
    Vs, vname = {}, {}

    def route(name, kind, fn_x, eta=None, **kw):
        # a column-major buffer of its own (V0 is column-major already: V0.t().contiguous() is V0)
        Vs[name] = torch.empty((k, d), dtype=torch.float32, device=dev).t()
        vname[len(vname)] = name
        eta = ETAS[kind] if eta is None else eta

        def fn():
            Vs[name].copy_(V0)
            linalg.oja_steps(fn_x(), Vs[name], eta, b, orth, check=False, **kw)
        return fn
    ways = {}
    for kind, x in xs.items():
        ways[f"a_{kind}_centred_in_place"] = route(f"a_{kind}", kind, lambda x=x: x, algo="two_pass",
                                                   center=cs[kind])
        ways[f"b_{kind}_materialise_two_pass"] = route(
            f"b_{kind}", kind, lambda x=x, c=cs[kind]: (x.double() - c).float(), algo="two_pass")
    # uncentred bytes: the mean direction dominates (eigenvalue about 128^2 d); a step size with
    # eta lambda about 1 keeps the float32 CholQR, and with it the bits check, meaningful
    eta_u = 1.0 / (128.0 ** 2 * d)
    ways["u8_bytes_in_place"] = route("u8_bytes", "u8", lambda: xs["u8"], eta=eta_u, algo="two_pass")
    ways["u8_widen_two_pass"] = route("u8_widen_tp", "u8", lambda: xs["u8"].float(), eta=eta_u,
                                      algo="two_pass")
    ways["u8_widen_auto"] = route("u8_widen_auto", "u8", lambda: xs["u8"].float(), eta=eta_u, algo="auto")
    vname = dict(zip(ways, vname.values()))  # route -> the name of its basis
    res = interleaved(ways, steps, warmup, trials, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    linalg.oja_check(dev, b, d, k)  # u8_widen_auto's resident hand-offs: none timed out
    out = {"b": b, "d": d, "k": k, "batches": nb, "orth_every": orth,
           "u8_widen_auto_is_resident": bool(b == 4096 and d % 512 == 0 and d <= 3072 and k <= 32)}
    for name in ways:
        per_batch = [t / nb for t in res[name]]
        out[f"{name}_ms_per_batch"] = statistics.median(per_batch)
        out[f"{name}_ms_per_batch_min_max"] = [min(per_batch), max(per_batch)]
        out[f"{name}_ms_per_batch_trials"] = per_batch
        out[f"{name}_nonfinite"] = int((~torch.isfinite(Vs[vname[name]])).sum())
    for kind in xs:
        a, bb = f"a_{kind}_centred_in_place", f"b_{kind}_materialise_two_pass"
        out[f"{kind}_a_over_b"] = out[f"{a}_ms_per_batch"] / out[f"{bb}_ms_per_batch"]
        out[f"{kind}_a_faster_than_b_beyond_spread"] = (out[f"{a}_ms_per_batch_min_max"][1]
                                                        < out[f"{bb}_ms_per_batch_min_max"][0])
        out[f"{kind}_a_bits_equal_b"] = bool(torch.equal(Vs[f"a_{kind}"], Vs[f"b_{kind}"]))
        out[f"{kind}_a_finite"] = bool(torch.isfinite(Vs[f"a_{kind}"]).all())
        # bytes of X a batch reads in (a): both passes
        out[f"{kind}_a_x_bytes_per_batch"] = 2 * ELEM_BYTES[kind] * b * d
        out[f"{kind}_a_frac_hbm"] = (out[f"{kind}_a_x_bytes_per_batch"]
                                     / (out[f"{a}_ms_per_batch"] * 1e-3) / 8e12)
    out["u8_bytes_over_widen_auto"] = out["u8_bytes_in_place_ms_per_batch"] / out["u8_widen_auto_ms_per_batch"]
    out["u8_bytes_faster_than_widen_auto_beyond_spread"] = (
        out["u8_bytes_in_place_ms_per_batch_min_max"][1] < out["u8_widen_auto_ms_per_batch_min_max"][0])
    out["u8_widen_auto_faster_than_bytes_beyond_spread"] = (
        out["u8_widen_auto_ms_per_batch_min_max"][1] < out["u8_bytes_in_place_ms_per_batch_min_max"][0])
    out["u8_bytes_bits_equal_widen_two_pass"] = bool(torch.equal(Vs["u8_bytes"], Vs["u8_widen_tp"]))
    out["u8_bytes_finite"] = bool(torch.isfinite(Vs["u8_bytes"]).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x3072x32x64x8,4096x8192x64x16x8",
                    help="comma list of b x d x k x batches x orth_every")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oja_centered.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("oja_centered_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    res = {"tool": "oja_centered_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "trials": a.trials,
           "timing": "HIP events around whole calls (all batches, both re-orthonormalisations and, "
                     "in the (b) and widen routes, the materialised float32 tensor included), per "
                     "batch; median and min/max of the trials, the routes alternated, clocks as "
                     "found",
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
    bad = [f"{s['b']}x{s['d']} {kind}" for s in res["shapes"] for kind in ETAS
           if not (s[f"{kind}_a_bits_equal_b"] and s[f"{kind}_a_finite"])]
    bad += [f"{s['b']}x{s['d']} u8 bytes" for s in res["shapes"]
            if not (s["u8_bytes_bits_equal_widen_two_pass"] and s["u8_bytes_finite"])]
    if bad:
        raise SystemExit(f"oja_centered_bench: in-place and materialised routes differ in bits, or "
                         f"are not finite: {bad}")


if __name__ == "__main__":
    main()
