"""C ABI of the uint8 centred-PCA entry points (integer column sums, centred exact covariance,
fused byte transform): declared, exported, bound, workspace queries answer, bad arguments are
rejected with a telling message before any GPU work (CPU)."""
import pytest

from distributed_eigenspaces_amd import _lib

SYMBOLS = ["deig_colsum_u8", "deig_colsum_u8_workspace", "deig_syrk_u8_centered",
           "deig_syrk_u8_centered_workspace", "deig_pca_transform_u8",
           "deig_pca_transform_u8_workspace"]
RAW, GRAY = _lib.DEIG_U8_RAW, _lib.DEIG_U8_GRAY3


def test_symbols_declared_exported_and_bound():
    L = _lib.lib()
    hdr = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in hdr, f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert s in _lib.SIGNATURES, f"no ctypes signature for {s}"
    assert L.deig_version() == 0x000600  # additive entry points


@pytest.mark.parametrize("n,d", [(1, 4), (60000, 3072), (1 << 21, 8192)])
def test_workspace_queries(n, d):
    L = _lib.lib()
    assert L.deig_colsum_u8_workspace(n, d) >= d * 8 > 0  # the integer sums
    for mode in (RAW, GRAY):
        wc = L.deig_syrk_u8_centered_workspace(n, d, mode)
        assert wc >= L.deig_syrk_u8_workspace(n, d, mode) + d * 8 > 0  # plus the centre terms
    for k in (1, 64, 256):
        kp = (k + 15) // 16 * 16
        assert L.deig_pca_transform_u8_workspace(n, d, k) >= d * kp * 4 > 0  # the packed W image


def _align(x, a):
    return (x + a - 1) // a * a


# the packed W image (dpad x kp floats) and the padded mean (dpad doubles), each a 256-byte
# aligned slice, dpad = d rounded up to a super-chunk of 128 features
@pytest.mark.parametrize("n,d,k,want", [(1, 4, 1, 9216), (1000, 260, 17, 52224),
                                        (1 << 20, 3072, 256, 3170304)])
def test_transform_workspace_is_exact(n, d, k, want):
    L = _lib.lib()
    dpad, kp = _align(d, 128), _align(k, 16)
    assert want == _align(dpad * kp * 4, 256) + _align(dpad * 8, 256)
    assert L.deig_pca_transform_u8_workspace(n, d, k) == want
    assert L.deig_pca_transform_u8_workspace(n, d, 0) == 0
    assert L.deig_pca_transform_u8_workspace(n, d, 257) == 0


# NULL pointers everywhere: the argument rules come first, nothing touches a GPU
def _colsum(n=8, d=16, ldx=16, mode=RAW):
    return _lib.lib().deig_colsum_u8(None, n, d, ldx, mode, None, None, 0, None)


def _centered(n=8, d=16, ldx=16, mode=RAW):
    return _lib.lib().deig_syrk_u8_centered(None, n, d, ldx, mode, None, 1.0 / n, None, d, None, d,
                                            None, None, 0, None)


def _transform(n=8, d=16, ldx=16, mode=RAW, k=4, ldw=16, ldy=4):
    return _lib.lib().deig_pca_transform_u8(None, n, d, ldx, mode, None, None, k, ldw, None, ldy,
                                            None, None, None, 0, None)


@pytest.mark.parametrize("call", [_colsum, _centered, _transform])
@pytest.mark.parametrize("kw,word", [
    (dict(mode=7), "unknown mode 7"),
    (dict(d=18, ldx=20), "multiple of 4"),
    (dict(ldx=12), "ldx must be >= 16 bytes"),
    (dict(mode=GRAY, ldx=44), "ldx must be >= 48 bytes"),  # gray rows need 3 d bytes
    (dict(ldx=18), "multiple of 4"),
])
def test_shape_rules(call, kw, word):
    assert call(**kw) == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()


def test_centered_needs_an_output():
    assert _centered() == _lib.DEIG_EINVAL  # every shape rule holds, S and S64 both NULL
    assert "S and/or S64" in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(k=0), "k=0"),
    (dict(k=257, ldy=257), "k=257"),
    (dict(), "at least one output"),  # every shape rule holds, Y / resid / energy all NULL
])
def test_transform_bad_arguments(kw, word):
    assert _transform(**kw) == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()


def test_colsum_needs_pointers():
    assert _colsum() == _lib.DEIG_EINVAL  # every shape rule holds, X NULL
    assert "X must be" in _lib.last_error(), _lib.last_error()
