"""The bits of the covariance SYRK are pinned: ``deig_syrk_f32_ex`` must return exactly what
tests/golden/syrk_bits.npz recorded on an MI355X.  The kernels of csrc/syrk_split.hip and
csrc/syrk.hip use no atomics on data and add in a fixed order (the pacing counters only
delay blocks), so equal bits are what "behaviour unchanged" means for them; the accuracy of
the same op is tested against float64 in test_gpu_kernels.py and test_gpu_syrk_chunks.py.

The work decomposition (full phases, remainder items and their K segments, the tile order)
depends on the number of CUs, so every case skips on a device whose count differs from the
recorded one (256: an MI355X).  Each case is the smallest shape that reaches one path; with
G = 256 blocks, T tiles, q = T / G full phases, R = T mod G remainder tiles cut into nseg
K segments, NK K-tiles of 32 rows and a flush every 128 K-tiles:

* fused_small       3000 x 300, row stride 312: R = 3, nseg = 63, NK = 94 - every item a
                    remainder item of 1-2 K-tiles, a ragged last K-tile (3000 = 93 * 32 + 24),
                    features past d in both panels, the diagonal tiles' lo^2 path;
* fused_flush       32785 x 2048: R = 36, nseg = 7, NK = 1025 - ~146 K-tiles per segment, so
                    every item flushes once and reads the slab back; beta = 0;
* half_remainder    70197 x 2304: R = 45, nseg = 17, NK = 2194 - 129-130 K-tiles per segment:
                    two pacing points per item (remainder pacing against the round's item
                    count, XCD and chip-wide), a flush inside a remainder segment, diagonal
                    and off-diagonal tiles (all five wave variants of the half ring);
* half_full_compact 8200 x 6144: nt = 24, q = 1, R = 44, compact XCD-group order; NK = 257:
                    4 pacing points in the full phase, so the chip-wide level fires; flushes;
* half_full_super   8200 x 5700: nt = 23, q = 1, R = 20, super-tile order, d no multiple of 256;
* chunk_loop        4100 x 2304 through a workspace that holds 2080 rows of the split image
                    (two chunks: beta = 1 in the second), then 1030 more rows with
                    DEIG_SYRK_ACCUMULATE into the same S;
* fp32              100 x 256 on the f32-MFMA kernel (csrc/syrk.hip).

The fixture holds a SHA-256 of every case's input (a numpy that draws other numbers is
reported as that, not as a kernel failure), the CU count, a SHA-256 of the output's bytes
and the output's first 64 values.  To record it, run this module with the library to be
pinned first on the module path:

    PYTHONPATH=<checkout> python tests/test_gpu_syrk_bits.py [--out FILE]
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "syrk_bits.npz")

# name -> (n, d, row stride)
CASES = {
    "fused_small": (3000, 300, 312),
    "fused_flush": (32785, 2048, 2048),
    "half_remainder": (70197, 2304, 2304),
    "half_full_compact": (8200, 6144, 6144),
    "half_full_super": (8200, 5700, 5700),
    "chunk_loop": (4100 + 1030, 2304, 2304),
    "fp32": (100, 256, 256),
}
CHUNK_N, CHUNK_ROWS = 4100, 2080  # chunk_loop: rows of the first call, rows per chunk
NAMES = list(CASES)


def make_input(name):
    """The case's samples (n x row stride, float32) from its own seeded generator: a
    non-zero mean and values that are not bf16-exact, so the lo pieces matter."""
    n, _, ldx = CASES[name]
    rng = np.random.default_rng(31000 + NAMES.index(name))
    X = rng.standard_normal((n, ldx), dtype=np.float32)
    X *= np.float32(3.0)
    X += np.float32(1.0)
    return X


def digest(a):
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}:{a.shape}".encode())
    h.update(np.ascontiguousarray(a).data)
    return h.hexdigest()


def _syrk(L, x, alpha, S, code, ws_rows=None):
    """deig_syrk_f32_ex on the rows of x with a 0xFF-filled (NaN) workspace sized for
    ``ws_rows`` rows (default: all of them)."""
    from distributed_eigenspaces_amd import _lib
    n, d = x.shape
    nbytes = L.deig_syrk_workspace_ex(n if ws_rows is None else ws_rows, d, code & ~_lib.DEIG_SYRK_ACCUMULATE)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=x.device)
    rc = L.deig_syrk_f32_ex(x.data_ptr(), n, d, x.stride(0), ctypes.c_float(alpha), S.data_ptr(), S.stride(0),
                            code, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "deig_syrk_f32_ex")
    torch.cuda.synchronize()


def run_case(name, X, dev):
    """The case's S (d x d float32, host array)."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    n, d, _ = CASES[name]
    x = torch.from_numpy(X).to(dev)[:, :d]
    S = torch.full((d, d), float("nan"), dtype=torch.float32, device=dev)
    if name == "fp32":
        _syrk(L, x, 1.0 / n, S, _lib.DEIG_SYRK_FP32)
    elif name == "chunk_loop":
        assert L.deig_syrk_workspace_ex(CHUNK_ROWS, d, _lib.DEIG_SYRK_SPLIT3) < \
            L.deig_syrk_workspace_ex(CHUNK_N, d, _lib.DEIG_SYRK_SPLIT3), "one chunk would hold all rows"
        _syrk(L, x[:CHUNK_N], 1.0 / n, S, _lib.DEIG_SYRK_SPLIT3, ws_rows=CHUNK_ROWS)
        _syrk(L, x[CHUNK_N:], 1.0 / n, S, _lib.DEIG_SYRK_SPLIT3 | _lib.DEIG_SYRK_ACCUMULATE)
    else:
        _syrk(L, x, 1.0 / n, S, _lib.DEIG_SYRK_SPLIT3)
    return S.cpu().numpy()


def cu_count(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("name", NAMES)
def test_bits_are_the_recorded_ones(name, cuda, recorded):
    if cu_count(cuda) != int(recorded["cus"]):
        pytest.skip(f"the work decomposition depends on the CU count: {cu_count(cuda)} here, "
                    f"{int(recorded['cus'])} recorded")
    X = make_input(name)
    assert digest(X) == str(recorded[name + "__in_sha256"]), \
        "the generated input differs from the recorded one (numpy's generator, not a kernel)"
    S = run_case(name, X, cuda)
    assert np.isfinite(S).all(), f"{name}: S holds non-finite values"
    head = S.reshape(-1)[:64].view(np.uint32)
    want = recorded[name + "__head"]
    assert np.array_equal(head, want), \
        f"{name}: the first 64 values differ: got {head.view(np.float32)}, recorded {want.view(np.float32)}"
    assert digest(S) == str(recorded[name + "__out_sha256"]), \
        f"{name}: S differs from the recorded bits (beyond its first 64 values)"


def record(path):
    dev = torch.device("cuda", 0)
    data = {"cus": np.int64(cu_count(dev))}
    for name in NAMES:
        X = make_input(name)
        data[name + "__in_sha256"] = np.str_(digest(X))
        first = run_case(name, X, dev)
        again = run_case(name, X, dev)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), f"{name}: two runs differ"
        assert np.isfinite(first).all(), name
        data[name + "__out_sha256"] = np.str_(digest(first))
        data[name + "__head"] = first.reshape(-1)[:64].view(np.uint32).copy()
        print(name, CASES[name], data[name + "__out_sha256"][:16], flush=True)
    np.savez_compressed(path, **data)
    print(f"recorded {len(NAMES)} cases on {torch.cuda.get_device_name(0)} "
          f"({int(data['cus'])} CUs): {path}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.path.append(ROOT)  # behind PYTHONPATH: the library to be pinned is found first
    record(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
