"""The covariance-free worker route against the explicit one, on the same tensor.

At each shape n x d (top k), for float32, bfloat16 and uint8 samples about their column mean:

* (free) ``linalg.topk_samples(x, k, center=c)``: the sample operator Y = Xc^T (Xc Q) / n in the
  solver (csrc/gram.hip, two reads of X per sweep, no d x d matrix);
* (explicit) the parent route: ``linalg.sigma_hat_centered`` (uint8:
  ``linalg.sigma_hat_u8_centered``, raw bytes) followed by ``linalg.topk_eigh``.  Shapes with
  d > 32768 run the free route only (the packed-sample covariance kernels stop there).

Reported per route: solver sweeps, ms per worker solve (covariance included for the explicit
route), and the peak device memory the route allocates beyond its inputs (torch's allocator
peak around one cold call, workspace cache emptied first); per sample type also ms per single
apply of the operator (``deig_gram_apply``, p the solver's subspace) and its achieved rate
against the fp32-MFMA work (4 n d p flops) and the bytes of X it reads twice.

The chunk comparison (``--chunk-shape``) times one apply with the workspace cut so that X is
worked through in 1, 2, 4, ... row chunks: whether a chunk small enough for the 256 MB
last-level cache makes the second read of X cheaper.  ``--ab-lib`` adds the same apply from a
measurement build of the library (``_build.build_library(defines=["-DDEIG_AB_GRAM_LINEAR_TILES"],
out=...)``: feature tiles in dispatch order instead of paired per XCD).

HIP events around whole calls, the routes alternated, median and min/max of ``--trials``
trials after ``--warmup`` calls, clocks as found.  Prints one JSON line and writes it to --out
(committed as profiles/topk_samples.json).

    python tools/topk_samples_bench.py [--shapes 1048576x3072x16,65536x16384x64,8192x32768x32,4096x65536x32]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_eigenspaces_amd import _lib, linalg, synthetic  # noqa: E402
from tools.oja_bf16_bench import interleaved  # noqa: E402

ELEM_BYTES = {"f32": 4, "bf16": 2, "u8": 1}
XTYPE = {"f32": "DEIG_F32", "bf16": "DEIG_BF16", "u8": "DEIG_U8"}
EXPLICIT_MAX_D = 32768


def make_samples(kind, n, d, k, dev):
    """Spiked rows (planted rank k, eigenvalues 8 s .. 4 s over unit noise), generated in
    blocks: float32 as they are, bfloat16 with a mean of 3, bytes clip(rint(128 + 16 x)).
    s = max(1, 16 d / n) keeps the spikes above the noise bulk of the sample covariance, whose
    edge is (1 + sqrt(d / n))^2: with fewer rows than features unit-scale spikes drown in it and
    no solver has a gap to converge on."""
    U = synthetic.planted_basis(d, k, seed=3, device=dev)
    s = max(1.0, 16.0 * d / n)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[kind]
    x = torch.empty((n, d), dtype=dt, device=dev)
    step = max(1, (1 << 27) // d)
    for i, lo in enumerate(range(0, n, step)):
        blk = synthetic.spiked_samples(min(step, n - lo), U, seed=11 + i, theta_hi=8.0 * s, theta_lo=4.0 * s)
        hi = lo + blk.shape[0]
        if kind == "f32":
            x[lo:hi] = blk
        elif kind == "bf16":
            x[lo:hi] = (blk + 3).to(torch.bfloat16)
        else:
            x[lo:hi] = torch.clip(torch.round(128 + 16 * blk), 0, 255).to(torch.uint8)
    return x


def column_mean(x):
    if x.dtype == torch.uint8:
        return linalg.column_sums_u8(x, "raw") / x.shape[0]
    return linalg.column_sums(x) / x.shape[0]


def explicit_route(x, k, c):
    if x.dtype == torch.uint8:
        S = linalg.sigma_hat_u8_centered(x, center=c, mode="raw")
    else:
        S = linalg.sigma_hat_centered(x, center=c)
    if isinstance(S, tuple):
        S = S[0]
    return linalg.topk_eigh(S, k, check_finite=False)


def peak_extra_bytes(fn, dev):
    """Peak device memory fn() allocates beyond what is live now (workspace cache emptied)."""
    linalg._ws.bufs.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del r
    return int(peak)


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)], "ms_trials": ms}


def bind(path):
    """A second copy of the library (a measurement build), bound from the same header."""
    L = ctypes.CDLL(path)
    for name in ("deig_gram_apply", "deig_gram_apply_workspace"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def apply_fn(L, x, kind, c, p, dev, ws_bytes=None):
    """fn() = one deig_gram_apply of library L on x about c with a d x p basis."""
    n, d = x.shape
    xt = getattr(_lib, XTYPE[kind])
    g = torch.Generator(device="cpu").manual_seed(5)
    Q = torch.linalg.qr(torch.randn(d, p, generator=g, dtype=torch.float32))[0].contiguous().to(dev)
    Y = torch.empty((d, p), dtype=torch.float32, device=dev)
    nbytes = int(L.deig_gram_apply_workspace(n, d, p, xt)) if ws_bytes is None else int(ws_bytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fn():
        rc = L.deig_gram_apply(x.data_ptr(), xt, n, d, x.stride(0), c.data_ptr(), 1.0 / n, Q.data_ptr(), p, p,
                               Y.data_ptr(), p, ws.data_ptr(), nbytes, stream)
        if rc:
            raise SystemExit(f"deig_gram_apply failed: {rc}")
    fn.keep = (Q, Y, ws)
    return fn


def chunk_bytes(L, n_rows, d, p, xt):
    """A workspace that holds a chunk of n_rows rows (Zt, the transform's image, the widest
    split-K slabs) - generous by the slabs, so the chunk is n_rows or slightly more."""
    ks_max = -(-4 * 256 // -(-d // 64))
    return n_rows * p * 4 + int(L.deig_gram_apply_workspace(1, d, p, xt)) + max(ks_max, 1) * d * p * 4 + 4096


def run_shape(n, d, k, a, dev, ab):
    out = {"n": n, "d": d, "k": k, "kinds": {}}
    p = linalg.default_subspace(d, k)
    out["p"] = p
    L = _lib.lib()
    for kind in a.kinds.split(","):
        x = make_samples(kind, n, d, k, dev)
        c = column_mean(x)
        res = {}
        ways = {"free": lambda: linalg.topk_samples(x, k, center=c)}
        if d <= EXPLICIT_MAX_D:
            ways["explicit"] = lambda: explicit_route(x, k, c)
        last = {}
        timed = {name: (lambda name=name, fn=fn: last.__setitem__(name, fn())) for name, fn in ways.items()}
        ms = interleaved(timed, 1, a.warmup, a.trials, torch.cuda.current_stream(dev))
        for name in ways:
            res[name] = stats(ms[name])
            res[name]["sweeps"] = int(last[name].sweeps)
            res[name]["converged"] = bool(last[name].converged)
            res[name]["resid"] = float(last[name].resid)
        if "explicit" in ways:
            res["subspace_distance_free_vs_explicit"] = float(
                linalg.projector_distance(last["free"].V, last["explicit"].V))
            res["free_over_explicit"] = res["free"]["ms"] / res["explicit"]["ms"]
        last.clear()
        for name, fn in ways.items():
            res[name]["peak_extra_bytes"] = peak_extra_bytes(fn, dev)
        fns = {"apply": apply_fn(L, x, kind, c, p, dev)}
        if ab is not None:
            fns["apply_linear_tiles"] = apply_fn(ab, x, kind, c, p, dev)
        ms = interleaved(fns, a.apply_steps, a.warmup, a.trials, torch.cuda.current_stream(dev))
        for name in fns:
            res[name] = stats(ms[name])
        t = res["apply"]["ms"] * 1e-3
        res["apply"]["fp32_mfma_tflops"] = 4.0 * n * d * p / t / 1e12
        res["apply"]["x_bytes_per_s_tb"] = 2.0 * n * d * ELEM_BYTES[kind] / t / 1e12
        res["apply"]["workspace_bytes"] = int(L.deig_gram_apply_workspace(n, d, p, getattr(_lib, XTYPE[kind])))
        res["free"]["workspace_query_bytes"] = int(L.deig_topk_samples_workspace(
            n, d, k, p, getattr(_lib, XTYPE[kind]), None))
        out["kinds"][kind] = res
        print(f"[topk_samples_bench] {n}x{d} k={k} {kind}: done", file=sys.stderr, flush=True)
        del x, fns
        torch.cuda.empty_cache()
    return out


def run_chunks(n, d, k, a, dev):
    """One apply at n x d with the workspace cut to 1, 2, 4, ... chunks of rows."""
    out = {"n": n, "d": d, "k": k, "kinds": {}}
    p = linalg.default_subspace(d, k)
    out["p"] = p
    L = _lib.lib()
    for kind in a.kinds.split(","):
        x = make_samples(kind, n, d, k, dev)
        c = column_mean(x)
        xt = getattr(_lib, XTYPE[kind])
        fns = {}
        m = 1
        while n // m >= 1024 and m <= 64:
            fns[f"chunks_{m}"] = apply_fn(L, x, kind, c, p, dev, chunk_bytes(L, -(-n // m), d, p, xt))
            m *= 2
        fns["recommended"] = apply_fn(L, x, kind, c, p, dev)
        ms = interleaved(fns, a.apply_steps, a.warmup, a.trials, torch.cuda.current_stream(dev))
        res = {name: stats(v) for name, v in ms.items()}
        for name in res:
            if name.startswith("chunks_"):
                res[name]["chunk_sample_bytes"] = -(-n // int(name[7:])) * d * ELEM_BYTES[kind]
        out["kinds"][kind] = res
        del x, fns
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576x3072x16,65536x16384x64,8192x32768x32,4096x65536x32",
                    help="comma list of n x d x k")
    ap.add_argument("--chunk-shape", default="65536x16384x64", help="n x d x k of the chunk comparison ('' = none)")
    ap.add_argument("--kinds", default="f32,bf16,u8")
    ap.add_argument("--apply-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--ab-lib", default="", help="a -DDEIG_AB_GRAM_LINEAR_TILES build of the library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_samples.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_samples_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    ab = bind(a.ab_lib) if a.ab_lib else None
    res = {"tool": "topk_samples_bench", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "trials": a.trials, "apply_steps": a.apply_steps,
           "timing": "HIP events around whole calls (explicit: covariance + solve; free: the solve), the "
                     "routes alternated; median and min/max of the trials, clocks as found",
           "shapes": [], "chunks": None}
    for shape in a.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        res["shapes"].append(run_shape(n, d, k, a, dev, ab))
    if a.chunk_shape:
        n, d, k = (int(v) for v in a.chunk_shape.split("x"))
        res["chunks"] = run_chunks(n, d, k, a, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = [f"{s['n']}x{s['d']} {kind} {route}" for s in res["shapes"] for kind, r in s["kinds"].items()
           for route in ("free", "explicit") if route in r and not r[route]["converged"]]
    if bad:
        raise SystemExit(f"topk_samples_bench: not converged: {bad}")


if __name__ == "__main__":
    main()
