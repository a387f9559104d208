"""The bits of every kernel that reads a sample "as it lies" (csrc/sample_src.hpp: float32,
bfloat16 or a raw byte, optionally centred as fl32((double)x - centre[j])) are pinned: the
two-pass Oja kernels and deig_gram_apply must return exactly what tests/golden/sample_bits.npz
recorded on an MI355X.  The kernels use no atomics and add in a fixed order, so equal bits are
what "behaviour unchanged" means for them; their accuracy is tested against float64 in
test_gpu_oja_centered.py, test_gpu_oja_bf16.py and test_gpu_gram_apply.py, and the packed
transform kernels have their own fixture (test_gpu_transform_bits.py).

Samples: float32 100 + 3 randn; bfloat16 the same values with their low 16 bits cleared; bytes
uniform in 0..255.  The centre is the float64 column mean plus 0.37, so that it is no sample's
value.  X has a row stride of d plus one load group (4 elements, 8 of bfloat16).

Oja cases (b, d, k, nb, orth_every), each centred and uncentred through the C entry points
(float32 uncentred: deig_oja_steps_ex with DEIG_OJA_TWO_PASS; bfloat16 uncentred: both
deig_oja_steps_bf16 and deig_oja_steps_centered with a NULL centre; everything else
deig_oja_steps_centered): SMALL12 the min(k + 4, d - 4) clamp (float32 and bytes: d % 8 == 4);
ONE b = 1, k = 1; MID empty wave slices, NB = 2; NB3; BIG the steady loop and the tail of both
passes, NB = 4.  The step size keeps eta lambda_max near 1 (0.02 / variance about a centre,
1 / (mean^2 d) without one), so every recorded basis is finite.

deig_gram_apply cases (n, d, p), each for the three types, centred and uncentred: (1, 16, 16)
one row; (31, 20, 16) a partly filled feature tile and chunk; (65, 68, 48) a second feature
tile, NB = 3; (97, 260, 128) NB = 8; (2048, 64, 16) the split-K reduce; (200, 132, 80) on the
workspace of 67 rows: three row chunks, the beta = 1 path.  bfloat16 rows come in groups of 8,
so its d is the next multiple of 8 (24, 72, 264, 136).  The split-K case depends on the number
of CUs: it is recorded only if the split gives more than one slice and skips on a device whose
count differs from the recorded one.

The fixture holds a SHA-256 of every case's inputs (a numpy that draws other numbers is
reported as that, not as a kernel failure), the CU count, the raw bits of every output of at
most 64 KiB and a SHA-256 of larger ones.  To record it, run this module with the library to
be pinned first on the module path:

    PYTHONPATH=<checkout> python tests/test_gpu_sample_bits.py [--out FILE]

The Python layer's operand preparation (linalg._packed_samples) is tested at the end, on the
device, without a fixture."""
import ctypes
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sample_bits.npz")
RAW_LIMIT = 64 * 1024
OFFSET = 0.37
KINDS = ("f32", "bf16", "u8")
GROUP = {"f32": 4, "bf16": 8, "u8": 4}
MEAN = {"f32": 100.0, "bf16": 100.0, "u8": 127.5}
VARIANCE = {"f32": 9.0, "bf16": 9.0, "u8": (256.0 ** 2 - 1.0) / 12.0}
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}

OJA_SHAPES = {"SMALL12": (50, 12, 3, 3, 2), "ONE": (1, 40, 1, 1, 1), "MID": (272, 264, 17, 5, 2),
              "NB3": (96, 520, 33, 4, 3), "BIG": (2600, 2816, 64, 2, 1)}
GRAM_SHAPES = [(1, 16, 16, None), (31, 20, 16, None), (65, 68, 48, None), (97, 260, 128, None),
               (2048, 64, 16, None), (200, 132, 80, 67)]  # (n, d, p, rows of the workspace query)
SPLIT_K = (2048, 64, 16)


def _cases():
    """(id, op, kind, shape, centred, entry) in a fixed order; the index seeds the generator of
    the (op, kind, shape) the case belongs to."""
    out = []
    for name, shape in OJA_SHAPES.items():
        for kind in KINDS:
            if name == "SMALL12" and kind == "bf16":
                continue
            for centred in (False, True):
                if centred:
                    entries = ("centered",)
                else:
                    entries = {"f32": ("ex",), "bf16": ("bf16", "centered"), "u8": ("centered",)}[kind]
                for entry in entries:
                    out.append((f"oja_{kind}_{name}_{entry}" + ("_c" if centred else ""), "oja", kind, shape,
                                centred, entry))
    for n, d, p, rows in GRAM_SHAPES:
        for kind in KINDS:
            dk = -(-d // GROUP[kind]) * GROUP[kind]
            for centred in (False, True):
                out.append((f"gram_{kind}_{n}x{dk}x{p}" + (f"_ws{rows}" if rows else "") + ("_c" if centred else ""),
                            "gram", kind, (n, dk, p, rows), centred, "gram_apply"))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def _seed(op, kind, shape):
    keys = sorted({(c[1], c[2], c[3][:3]) for c in CASES})
    return 31000 + keys.index((op, kind, shape[:3]))


@functools.lru_cache(maxsize=4)
def make_inputs(op, kind, shape):
    """The inputs that the centred and the uncentred cases of one (op, kind, shape) share, from
    their own seeded generator.  Never written to."""
    rng = np.random.default_rng(_seed(op, kind, shape))
    if op == "oja":
        b, d, k, nb, _ = shape
        n, cols = nb * b, k
    else:
        n, d, cols = shape[:3]
    ld = d + GROUP[kind]
    if kind == "u8":
        X = rng.integers(0, 256, (n, ld), dtype=np.uint8)
    else:
        X = np.float32(100.0) + np.float32(3.0) * rng.standard_normal((n, ld), dtype=np.float32)
        if kind == "bf16":  # bf16 values held as float32: the low 16 bits cleared
            X.view(np.uint32)[...] &= np.uint32(0xffff0000)
    centre = X[:, :d].astype(np.float64).mean(0) + OFFSET
    G = rng.standard_normal((d, cols))
    if op == "oja":
        G = np.linalg.qr(G)[0]
    inputs = {"X": X, "centre": centre, "B": np.ascontiguousarray(G.astype(np.float32))}
    return inputs


def digest(arrays):
    h = hashlib.sha256()
    for name, a in arrays.items():
        h.update(f"{name}:{a.dtype.str}:{a.shape}".encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=4)
def _input_digest(op, kind, shape):
    return digest(make_inputs(op, kind, shape))


def _xtype(kind):
    from distributed_eigenspaces_amd import _lib
    return {"f32": _lib.DEIG_F32, "bf16": _lib.DEIG_BF16, "u8": _lib.DEIG_U8}[kind]


def _device_samples(inputs, kind, dev):
    X = torch.from_numpy(inputs["X"]).to(dev)
    return X.to(torch.bfloat16) if kind == "bf16" else X  # exact: make_inputs cleared the low bits


def run_case(case, dev):
    """The case's output as a float32 tensor: V (d x k, column-major) or Y (d x p)."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    _, op, kind, shape, centred, entry = case
    inputs = make_inputs(op, kind, shape[:3] if op == "gram" else shape)
    X = _device_samples(inputs, kind, dev)
    ldx = X.stride(0)
    c = torch.from_numpy(inputs["centre"]).to(dev) if centred else None
    cptr = None if c is None else c.data_ptr()
    B = torch.from_numpy(inputs["B"]).to(dev)
    if op == "oja":
        b, d, k, nb, orth = shape
        eta = 0.02 / VARIANCE[kind] if centred else 1.0 / (MEAN[kind] ** 2 * d)
        V = B.t().contiguous().t()  # column-major, ldv = d
        nbytes = L.deig_oja_workspace(b, d, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tail = (ctypes.c_float(eta), V.data_ptr(), k, d, orth)
        if entry == "ex":
            rc = L.deig_oja_steps_ex(X.data_ptr(), nb, b, d, ldx, *tail, _lib.DEIG_OJA_TWO_PASS,
                                     ws.data_ptr(), nbytes, None)
        elif entry == "bf16":
            rc = L.deig_oja_steps_bf16(X.data_ptr(), nb, b, d, ldx, *tail, ws.data_ptr(), nbytes, None)
        else:
            rc = L.deig_oja_steps_centered(X.data_ptr(), _xtype(kind), nb, b, d, ldx, cptr, *tail,
                                           ws.data_ptr(), nbytes, None)
        out = V.t()  # the k x d buffer as it lies
    else:
        n, d, p, rows = shape
        nbytes = L.deig_gram_apply_workspace(rows or n, d, p, _xtype(kind))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.full((d, p), float("nan"), dtype=torch.float32, device=dev)
        rc = L.deig_gram_apply(X.data_ptr(), _xtype(kind), n, d, ldx, cptr, ctypes.c_float(1.0 / n),
                               B.data_ptr(), p, p, out.data_ptr(), p, ws.data_ptr(), nbytes, None)
    assert rc == _lib.DEIG_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), case[0]
    return out


def cu_count(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def split_k_slices(d, p, n):
    """Slices of the second product's split-K: the skinny GEMM's rule, read off its slab size."""
    from distributed_eigenspaces_amd import _lib
    return max(1, _lib.lib().deig_gemm_skinny_workspace(d, p, n) // (4 * d * p))


def bits_of(out):
    """("raw", uint32 array) for an output of at most RAW_LIMIT bytes, else ("sha256", hex)."""
    a = out.contiguous().cpu().numpy().view(np.uint32)
    return ("raw", a) if a.nbytes <= RAW_LIMIT else ("sha256", hashlib.sha256(a.tobytes()).hexdigest())


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_bits_are_the_recorded_ones(index, cuda, recorded):
    case = CASES[index]
    cid, op, kind, shape = case[:4]
    key = shape[:3] if op == "gram" else shape
    if op == "gram" and shape[:3] == SPLIT_K and cu_count(cuda) != int(recorded["cus"]):
        pytest.skip(f"split-K slices depend on the CU count: {cu_count(cuda)} here, "
                    f"{int(recorded['cus'])} recorded")
    assert _input_digest(op, kind, key) == str(recorded[cid + "__sha256"]), \
        "the generated inputs differ from the recorded ones (numpy's generator, not a kernel)"
    how, got = bits_of(run_case(case, cuda))
    if how == "raw":
        want = recorded[cid + "__out"]
        assert got.shape == want.shape
        assert np.array_equal(got, want), \
            f"{cid}: {int((got != want).sum())} of {want.size} values differ in their bits"
    else:
        assert got == str(recorded[cid + "__out_sha256"]), f"{cid}: the output's hash differs"


def record(path):
    dev = torch.device("cuda", 0)
    data = {"cus": np.int64(cu_count(dev))}
    n, d, p = SPLIT_K
    split = split_k_slices(d, p, n) > 1
    for case in CASES:
        cid, op, kind, shape = case[:4]
        if op == "gram" and shape[:3] == SPLIT_K and not split:
            print(f"{cid}: one slice on this device, not recorded")
            continue
        key = shape[:3] if op == "gram" else shape
        data[cid + "__sha256"] = np.str_(_input_digest(op, kind, key))
        how, first = bits_of(run_case(case, dev))
        _, again = bits_of(run_case(case, dev))
        if how == "raw":
            assert np.array_equal(first, again), f"{cid}: two runs differ"
            data[cid + "__out"] = first
        else:
            assert first == again, f"{cid}: two runs differ"
            data[cid + "__out_sha256"] = np.str_(first)
    np.savez_compressed(path, **data)
    print(f"recorded {len(CASES)} cases on {torch.cuda.get_device_name(0)} "
          f"({int(data['cus'])} CUs): {path}, {os.path.getsize(path)} bytes")


# ---------------------------------------------------------------- the Python layer, no fixture
def _samples(kind, n, cols, dev, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "u8":
        return torch.randint(0, 256, (n, cols), generator=g, dtype=torch.uint8).to(dev)
    return (100 + 3 * torch.randn(n, cols, generator=g)).to(DTYPE[kind]).to(dev)


@pytest.mark.parametrize("kind", KINDS)
def test_packed_samples_reads_in_place_or_copies(kind, cuda):
    from distributed_eigenspaces_amd import _lib, linalg
    q, n, d = GROUP[kind], 9, 32
    wide = _samples(kind, n, d + 2 * q, cuda)
    # a row-strided view is read where it lies
    x = wide[:, :d]
    X, xtype, n_, d_, dp = linalg._packed_samples(x, "test", "X", 4)
    assert X.data_ptr() == x.data_ptr() and X.stride(0) == d + 2 * q
    assert (xtype, n_, d_, dp) == (_xtype(kind), n, d, d)
    assert xtype == getattr(_lib, {"f32": "DEIG_F32", "bf16": "DEIG_BF16", "u8": "DEIG_U8"}[kind])
    # a base offset by one element: a copy of the same dtype
    flat = _samples(kind, 1, n * (d + q) + 1, cuda).reshape(-1)
    x = flat[1:].reshape(n, d + q)[:, :d]
    X, _, _, _, dp = linalg._packed_samples(x, "test", "X", 4)
    assert X.data_ptr() != x.data_ptr() and X.dtype == x.dtype and dp == d
    assert X.data_ptr() % (4 if kind == "u8" else 16) == 0 and torch.equal(X[:, :d], x)
    # d not a multiple of the group: a zero-padded copy with dp columns
    x = wide[:, :d - 1]
    X, _, _, d_, dp = linalg._packed_samples(x, "test", "X", 4)
    assert d_ == d - 1 and dp == d and X.shape == (n, dp) and X.dtype == x.dtype
    assert torch.equal(X[:, :d - 1], x) and not X[:, d - 1:].any()
    # a column-strided view: a copy
    x = wide[:, ::2][:, :d // 2 // q * q]
    X, _, _, d_, dp = linalg._packed_samples(x, "test", "X", 4)
    assert X.data_ptr() != x.data_ptr() and X.stride(1) == 1 and torch.equal(X[:, :d_], x)


def test_float32_slices_equal_their_contiguous_copies(cuda):
    from distributed_eigenspaces_amd import linalg
    wide = _samples("f32", 70, 40, cuda)
    x = wide[:, :37]
    g = torch.Generator(device="cpu").manual_seed(6)
    W = torch.linalg.qr(torch.randn(37, 5, generator=g))[0].to(cuda)
    mean = x.double().mean(0)
    assert torch.equal(linalg.project(x, W), linalg.project(x.contiguous(), W))
    for got, want in zip(linalg.pca_transform(x, W, mean, residual=True, energy=True),
                         linalg.pca_transform(x.contiguous(), W, mean, residual=True, energy=True)):
        assert torch.equal(got, want)


if __name__ == "__main__":
    sys.path.append(ROOT)  # behind PYTHONPATH: the library to be pinned is found first
    record(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
