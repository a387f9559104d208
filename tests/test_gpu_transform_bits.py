"""The bits of the kernels built on the shared tile (csrc/skinny_tile.hpp) are pinned:
``pca_transform`` (float32 and bfloat16 samples), ``pca_transform_u8`` and ``gemm_skinny``
must return exactly what
tests/golden/transform_bits.npz recorded on an MI355X.  The kernels use no atomics and add
in a fixed order, so equal bits are what "behaviour unchanged" means for them; the accuracy
of the same calls is tested against float64 in test_gpu_pca_kernels.py,
test_gpu_u8_pca_kernels.py and test_gpu_skinny.py.

Each case is the smallest shape that reaches one path of the tile:

* pca_transform (n, d, k): (65, 36, 3) a row-tile tail, a partly filled second chunk and
  NB = 1 with its two accumulators; (129, 260, 17) k < kp, NB = 2; (63, 1028, 64) without a
  mean, the padded W stride; (65, 132, 256) NB = 16;
* pca_transform_u8: raw (65, 36, 3) four partly filled compute chunks, with and without a
  mean; raw (129, 260, 17) a last super-chunk of one chunk; raw (64, 132, 256); gray
  (129, 260, 17); raw (65, 136, 16) and (65, 140, 16) a last super-chunk of two and of
  three chunks; gray (65, 44, 3) without a mean, the dword tail load at three 4-feature
  groups;
* pca_transform of bfloat16 samples (the float32 values 100 + 3 randn with their low 16
  bits cleared, so the conversion is exact): (65, 72, 3) a row-tile tail, one whole
  super-chunk and one of 8 features, NB = 1 with its two accumulators; (129, 264, 17)
  k < kp, NB = 2; (63, 1032, 64) without a mean; (64, 136, 256) NB = 16; (65, 8, 3) a
  single super-chunk whose second chunk is all zeros, without a mean;
* gemm_skinny (M, N, K) on normal data with alpha = 1.5, beta = 0.5, both forms, split-K
  in two slices.  The split factor depends on the number of CUs, so these two skip on a
  device whose count differs from the recorded one.

The fixture holds a SHA-256 of every case's inputs (a numpy that draws other numbers is
reported as that, not as a kernel failure), the CU count and the raw bits of every output.
To record it, run this module with the library to be pinned first on the module path:

    PYTHONPATH=<checkout> python tests/test_gpu_transform_bits.py [--out FILE]
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "transform_bits.npz")

# (kind, shape, with mean) - kind "f32" / "raw" / "gray" / "bf16": (n, d, k); "gemmN" / "gemmT": (M, N, K)
CASES = [
    ("f32", (65, 36, 3), True),
    ("f32", (129, 260, 17), True),
    ("f32", (63, 1028, 64), False),
    ("f32", (65, 132, 256), True),
    ("raw", (65, 36, 3), True),
    ("raw", (129, 260, 17), True),
    ("raw", (64, 132, 256), True),
    ("gray", (129, 260, 17), True),
    ("raw", (65, 36, 3), False),
    ("gemmN", (130, 48, 516), False),
    ("gemmT", (132, 48, 516), False),
    ("bf16", (65, 72, 3), True),
    ("bf16", (129, 264, 17), True),
    ("bf16", (63, 1032, 64), False),
    ("bf16", (64, 136, 256), True),
    ("bf16", (65, 8, 3), False),
    ("raw", (65, 136, 16), True),
    ("raw", (65, 140, 16), True),
    ("gray", (65, 44, 3), False),
]
ALPHA, BETA = 1.5, 0.5


def case_id(case):
    kind, shape, with_mean = case
    return f"{kind}_{shape[0]}x{shape[1]}x{shape[2]}" + ("_mean" if with_mean else "")


def make_inputs(index, case):
    """The case's inputs, in order, from its own seeded generator."""
    kind, (a, b, c), with_mean = case
    rng = np.random.default_rng(20240 + index)
    if kind.startswith("gemm"):
        M, N, K = a, b, c
        return {"A": rng.standard_normal((K, M) if kind == "gemmT" else (M, K)).astype(np.float32),
                "B": rng.standard_normal((K, N)).astype(np.float32),
                "C": rng.standard_normal((M, N)).astype(np.float32)}
    n, d, k = a, b, c
    if kind in ("f32", "bf16"):
        X = (100.0 + 3.0 * rng.standard_normal((n, d))).astype(np.float32)
        if kind == "bf16":  # bf16 values held as float32: the low 16 bits cleared
            X.view(np.uint32)[...] &= np.uint32(0xffff0000)
        centre = 100.0
    else:
        X = rng.integers(0, 256, (n, 3 * d if kind == "gray" else d), dtype=np.uint8)
        centre = 127.5
    inputs = {"X": X, "W": rng.standard_normal((d, k)).astype(np.float32)}
    if with_mean:
        inputs["mean"] = centre + rng.standard_normal(d)
    return inputs


def digest(inputs):
    h = hashlib.sha256()
    for name, a in inputs.items():
        h.update(f"{name}:{a.dtype.str}:{a.shape}".encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(case, inputs, dev):
    """{name: float32 tensor} of the case's outputs."""
    from distributed_eigenspaces_amd import linalg
    kind = case[0]
    t = {name: torch.from_numpy(a).to(dev) for name, a in inputs.items()}
    if kind.startswith("gemm"):
        return {"C": linalg.gemm_skinny(t["A"], t["B"], kind == "gemmT", ALPHA, BETA, C=t["C"])}
    if kind in ("f32", "bf16"):
        if kind == "bf16":
            t["X"] = t["X"].to(torch.bfloat16)  # exact: make_inputs cleared the low bits
        out = linalg.pca_transform(t["X"], t["W"], t.get("mean"), residual=True, energy=True)
    else:
        out = linalg.pca_transform_u8(t["X"], t["W"], t.get("mean"), kind, residual=True,
                                      energy=True)
    return dict(zip(("Y", "resid", "energy"), out))


def cu_count(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("index", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_bits_are_the_recorded_ones(index, cuda, recorded):
    case = CASES[index]
    cid = case_id(case)
    inputs = make_inputs(index, case)
    assert digest(inputs) == str(recorded[cid + "__sha256"]), \
        "the generated inputs differ from the recorded ones (numpy's generator, not a kernel)"
    if case[0].startswith("gemm") and cu_count(cuda) != int(recorded["cus"]):
        pytest.skip(f"split-K slices depend on the CU count: {cu_count(cuda)} here, "
                    f"{int(recorded['cus'])} recorded")
    outs = run_case(case, inputs, cuda)
    assert sorted(outs) == (["C"] if case[0].startswith("gemm") else ["Y", "energy", "resid"])
    for name, got in outs.items():
        want = torch.from_numpy(recorded[f"{cid}__{name}"].view(np.int32)).to(cuda)
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        bits = got.contiguous().view(torch.int32)
        assert torch.equal(bits, want), \
            f"{cid} {name}: {int((bits != want).sum())} of {want.numel()} values differ in their bits"


def record(path):
    dev = torch.device("cuda", 0)
    data = {"cus": np.int64(cu_count(dev))}
    for index, case in enumerate(CASES):
        cid = case_id(case)
        inputs = make_inputs(index, case)
        data[cid + "__sha256"] = np.str_(digest(inputs))
        first = run_case(case, inputs, dev)
        again = run_case(case, inputs, dev)
        for name, got in first.items():
            assert torch.equal(got, again[name]), f"{cid} {name}: two runs differ"
            data[f"{cid}__{name}"] = got.cpu().numpy().view(np.uint32)
    np.savez_compressed(path, **data)
    print(f"recorded {len(CASES)} cases on {torch.cuda.get_device_name(0)} "
          f"({int(data['cus'])} CUs): {path}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.path.append(ROOT)  # behind PYTHONPATH: the library to be pinned is found first
    record(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
