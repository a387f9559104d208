"""The wide-data (dual) worker route against the covariance-free and the explicit one, on the
same tensor.

At each shape n x d (top k), for float32, bfloat16 and uint8 samples about their column mean:

* (dual) ``linalg.topk_dual(x, k, center=c)``: the n x n Gram matrix K = Xc Xc^T / n on the bf16
  MFMA (csrc/gram_nt.hip), its top-k by the explicit solver, one back-projection and the finish
  on the implicit operator;
* (free) ``linalg.topk_samples(x, k, center=c)`` from a cold start;
* (explicit) ``linalg.sigma_hat_centered`` (uint8: ``linalg.sigma_hat_u8_centered``, raw bytes)
  followed by ``linalg.topk_eigh``, where d <= 32768.

Reported per route: solver sweeps (dual: the finish's), ms per worker solve, and the peak device
memory the route allocates beyond its inputs.  The dual route's breakdown is timed on its
pieces, each a public call on the same tensors: ``gram_outer`` (prep + product), ``topk_eigh``
of K with the subspace the route uses (the n x n solve), the back-projection V0 = Xc^T Zt (the
second product of ``gram_apply``: one ``gram_apply`` on a d x round16(k) basis less the
``pca_transform`` that is its first product, a difference of two medians), the finish
(``topk_samples`` warm started with the back-projected start, formed once by torch), and the
remainder of the whole call (relayouts and the host's reads between the steps).

HIP events around whole calls, all routes and pieces alternated in one process, median and
min/max of ``--trials`` trials after ``--warmup`` calls, clocks as found.  A "win" is a median
outside the other route's min/max.  Prints one JSON line and writes it to --out (committed as
profiles/topk_dual.json); ``--append`` adds the shapes to the file that is there, so that each
shape can run as a process of its own under its own time limit.

    python tools/topk_dual_bench.py [--shapes 8192x32768x32,4096x65536x32,16384x16384x64,32768x8192x32]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_eigenspaces_amd import _lib, linalg  # noqa: E402
from tools.oja_bf16_bench import interleaved  # noqa: E402
from tools.topk_samples_bench import (EXPLICIT_MAX_D, XTYPE, column_mean, explicit_route,  # noqa: E402
                                      make_samples, peak_extra_bytes, stats)


def dual_start(x, c, K, k, p_n):
    """The route's start, formed by torch once: V0 = Xc^T U diag(sqrt(1 / (n lambda))), unit
    columns, from the top-k pairs of K (column-major, as a warm start is passed)."""
    n, d = x.shape
    r = linalg.topk_eigh(K, k, p=p_n, check_finite=False)
    U = r.V * torch.rsqrt(r.evals * n)[None, :]
    V0 = torch.zeros((d, k), dtype=torch.float32, device=x.device)
    step = max(1, (1 << 26) // d)
    for lo in range(0, n, step):
        blk = (x[lo:lo + step].to(torch.float64) - c[None, :]).to(torch.float32)
        V0 += blk.t() @ U[lo:lo + step]
    return V0.t().contiguous().t()


def first_product(x, Qk, c):
    """Zt = Xc Qk alone, the first product of gram_apply, by the type's fused transform."""
    if x.dtype == torch.uint8:
        return linalg.pca_transform_u8(x, Qk, mean=c, mode="raw")
    return linalg.pca_transform(x, Qk, mean=c)


def winner(res, a, b):
    """The route whose median lies below the other's fastest trial, else None."""
    if res[a]["ms"] < res[b]["ms_min_max"][0]:
        return a
    if res[b]["ms"] < res[a]["ms_min_max"][0]:
        return b
    return None


def run_shape(n, d, k, a, dev):
    out = {"n": n, "d": d, "k": k, "kinds": {}}
    p = linalg.default_subspace(d, k)
    p_n = linalg.default_subspace(n, k)
    out["p"], out["p_gram"] = p, p_n
    L = _lib.lib()
    for kind in a.kinds.split(","):
        x = make_samples(kind, n, d, k, dev)
        c = column_mean(x)
        K = linalg.gram_outer(x, center=c)
        V0 = dual_start(x, c, K, k, p_n)
        kp = -(-k // 16) * 16
        Qk = torch.zeros((d, kp), dtype=torch.float32, device=dev)
        Qk[:, :k] = V0
        ways = {"dual": lambda: linalg.topk_dual(x, k, center=c),
                "free": lambda: linalg.topk_samples(x, k, center=c)}
        if d <= EXPLICIT_MAX_D:
            ways["explicit"] = lambda: explicit_route(x, k, c)
        pieces = {"gram_outer": lambda: linalg.gram_outer(x, center=c),
                  "gram_solve": lambda: linalg.topk_eigh(K, k, p=p_n, check_finite=False),
                  "finish": lambda: linalg.topk_samples(x, k, center=c, q0=V0),
                  "apply_kp": lambda: linalg.gram_apply(x, Qk, center=c),
                  "transform_kp": lambda: first_product(x, Qk, c)}
        last = {}
        timed = {name: (lambda name=name, fn=fn: last.__setitem__(name, fn()))
                 for name, fn in {**ways, **pieces}.items()}
        ms = interleaved(timed, 1, a.warmup, a.trials, torch.cuda.current_stream(dev))
        res = {}
        for name in ways:
            res[name] = stats(ms[name])
            res[name]["sweeps"] = int(last[name].sweeps)
            res[name]["converged"] = bool(last[name].converged)
            res[name]["resid"] = float(last[name].resid)
        bd = {name: stats(ms[name]) for name in pieces}
        bd["gram_solve"]["sweeps"] = int(last["gram_solve"].sweeps)
        bd["finish"]["sweeps"] = int(last["finish"].sweeps)
        bd["back_projection_ms"] = bd["apply_kp"]["ms"] - bd["transform_kp"]["ms"]
        bd["remainder_ms"] = res["dual"]["ms"] - bd["back_projection_ms"] - sum(
            bd[name]["ms"] for name in ("gram_outer", "gram_solve", "finish"))
        # centred: three products (hi hi, hi lo, lo hi) of n^2 d flops each on the lower triangle
        bd["gram_outer"]["bf16_mfma_tflops"] = 3.0 * n * n * d / (bd["gram_outer"]["ms"] * 1e-3) / 1e12
        res["dual"]["breakdown"] = bd
        res["dual"]["workspace_query_bytes"] = int(L.deig_topk_dual_workspace(
            n, d, k, p, getattr(_lib, XTYPE[kind]), None))
        res["dual_vs_free"] = winner(res, "dual", "free")
        res["subspace_distance_dual_vs_free"] = float(linalg.projector_distance(last["dual"].V, last["free"].V))
        if "explicit" in ways:
            res["dual_vs_explicit"] = winner(res, "dual", "explicit")
        last.clear()
        for name, fn in ways.items():
            res[name]["peak_extra_bytes"] = peak_extra_bytes(fn, dev)
        out["kinds"][kind] = res
        print(f"[topk_dual_bench] {n}x{d} k={k} {kind}: done", file=sys.stderr, flush=True)
        del x, K, V0, Qk
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x32768x32,4096x65536x32,16384x16384x64,32768x8192x32",
                    help="comma list of n x d x k")
    ap.add_argument("--kinds", default="f32,bf16,u8")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--append", action="store_true", help="add the shapes to the file at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_dual.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_dual_bench: needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    res = {"tool": "topk_dual_bench", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "trials": a.trials,
           "timing": "HIP events around whole calls (explicit: covariance + solve; dual and free: the "
                     "solve), routes and pieces alternated; median and min/max of the trials, clocks as "
                     "found; a win is a median outside the other's min/max",
           "shapes": []}
    if a.append and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res["shapes"] = json.load(f)["shapes"]
    for shape in a.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        res["shapes"].append(run_shape(n, d, k, a, dev))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = [f"{s['n']}x{s['d']} {kind} {route}" for s in res["shapes"] for kind, r in s["kinds"].items()
           for route in ("dual", "free", "explicit") if route in r and not r[route]["converged"]]
    if bad:
        raise SystemExit(f"topk_dual_bench: not converged: {bad}")


if __name__ == "__main__":
    main()
