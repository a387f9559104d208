"""C ABI of the Procrustes average and the subspace distance: exported, bound, workspace
queries answer, bad arguments are rejected before any GPU work (CPU)."""
import pytest

from distributed_eigenspaces_amd import _lib

SYMBOLS = ["deig_procrustes_avg_f32", "deig_procrustes_workspace", "deig_subspace_dist_f32",
           "deig_subspace_dist_workspace"]


def test_symbols_exported_and_bound():
    L = _lib.lib()
    hdr = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in hdr, f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert s in _lib.SIGNATURES, f"no ctypes signature for {s}"
    assert L.deig_version() == 0x000600  # additive entry points


@pytest.mark.parametrize("d,mk,k", [(64, 20, 4), (8192, 512, 64), (16384, 8192, 128)])
def test_workspace_queries(d, mk, k):
    L = _lib.lib()
    kp = (k + 15) // 16 * 16
    ws = L.deig_procrustes_workspace(d, mk, k)
    # at least the reference image, the cross-Grams, the rotations and the average
    assert ws >= (2 * d * kp + 2 * mk * kp) * 4 > 0
    wd = L.deig_subspace_dist_workspace(d, k)
    assert wd >= 2 * d * kp * 4 > 0


def _avg(d, mk, k, iters):
    # NULL pointers everywhere: the argument rules come first, nothing touches a GPU
    return _lib.lib().deig_procrustes_avg_f32(None, d, mk, d, k, None, d, None, iters, None, d,
                                              None, None, None, 0, None)


@pytest.mark.parametrize("d,mk,k,iters,word", [
    (1024, 129 * 2, 129, 1, "k=129"),   # k > 128
    (8, 32, 16, 1, "exceed d"),         # k > d
    (64, 10, 4, 1, "multiple of k"),    # mk % k != 0
    (64, 20, 4, 0, "iters=0"),
    (64, 20, 4, 9, "iters=9"),
])
def test_procrustes_bad_arguments(d, mk, k, iters, word):
    assert _avg(d, mk, k, iters) == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()


def test_procrustes_null_stack_rejected():
    assert _avg(64, 20, 4, 1) == _lib.DEIG_EINVAL  # every shape rule holds, Wt is NULL
    assert "Wt" in _lib.last_error()


@pytest.mark.parametrize("d,k,word", [(1024, 129, "k=129"), (8, 16, "exceed d"), (66, 4, "d % 4")])
def test_subspace_dist_bad_arguments(d, k, word):
    rc = _lib.lib().deig_subspace_dist_f32(None, d, None, d, d, k, None, None, 0, None)
    assert rc == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()
