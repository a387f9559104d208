"""C ABI of the centred-PCA entry points (column sums, centred covariance, fused centred
transform): exported, bound, workspace queries answer, bad arguments are rejected before
any GPU work (CPU)."""
import pytest

from distributed_eigenspaces_amd import _lib

SYMBOLS = ["deig_colsum", "deig_colsum_workspace", "deig_syrk_centered",
           "deig_syrk_centered_workspace", "deig_pca_transform_f32", "deig_pca_transform_workspace"]


def test_symbols_exported_and_bound():
    L = _lib.lib()
    hdr = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in hdr, f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert s in _lib.SIGNATURES, f"no ctypes signature for {s}"
    assert L.deig_version() == 0x000600  # additive entry points


@pytest.mark.parametrize("n,d,k", [(1, 4, 1), (60000, 3072, 64), (1 << 21, 8192, 256)])
def test_workspace_queries(n, d, k):
    L = _lib.lib()
    kp = (k + 15) // 16 * 16
    assert L.deig_pca_transform_workspace(n, d, k) >= d * kp * 4 > 0  # the packed W image
    assert L.deig_colsum_workspace(n, d) >= min(n, 128) * d * 8 > 0   # the row-group partials
    for xtype in (_lib.DEIG_F32, _lib.DEIG_F64):
        wc = L.deig_syrk_centered_workspace(n, d, xtype)
        # the deig_syrk_shift pipeline (fp32 copy of the shard included) plus delta
        assert wc >= L.deig_syrk_shift_workspace(n, d, xtype) + d * 8 > 0


def _transform(n=8, d=16, ldx=16, k=4, ldw=16, ldy=4):
    # NULL pointers everywhere: the argument rules come first, nothing touches a GPU
    return _lib.lib().deig_pca_transform_f32(None, n, d, ldx, None, None, k, ldw, None, ldy, None,
                                             None, None, 0, None)


@pytest.mark.parametrize("kw,word", [
    (dict(k=0), "k=0"),
    (dict(k=257, ldy=257), "k=257"),
    (dict(ldx=12), "ldx must be >= d"),
    (dict(ldx=18), "ldx % 4"),
    (dict(), "at least one output"),  # every shape rule holds, Y / resid / energy all NULL
])
def test_transform_bad_arguments(kw, word):
    assert _transform(**kw) == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()


def _centered(xtype, n=8, d=16):
    return _lib.lib().deig_syrk_centered(None, xtype, n, d, d, None, 1.0 / n, None, d, None, d, None,
                                         None, 0, None)


def test_centered_bad_arguments():
    assert _centered(7) == _lib.DEIG_EINVAL
    assert "unknown element type 7" in _lib.last_error(), _lib.last_error()
    assert _centered(_lib.DEIG_F32) == _lib.DEIG_EINVAL  # S64 and S both NULL
    assert "S64 and/or S" in _lib.last_error(), _lib.last_error()


def test_colsum_bad_arguments():
    rc = _lib.lib().deig_colsum(None, 7, 8, 16, 16, None, None, 0, None)
    assert rc == _lib.DEIG_EINVAL
    assert "unknown element type 7" in _lib.last_error(), _lib.last_error()
