"""C ABI of the bf16 entry points (covariance of bf16 samples as they are, fused bf16
transform, DEIG_BF16 as an element type of the column passes): declared, exported, bound from
the header, workspace queries answer, bad arguments are rejected with a message naming the
rule before any GPU work (CPU)."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

SYMBOLS = ["deig_syrk_bf16", "deig_syrk_bf16_workspace", "deig_pca_transform_bf16",
           "deig_pca_transform_bf16_workspace"]
PTR = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced


def test_symbols_declared_exported_and_bound():
    L = _lib.lib()
    hdr = _lib.header_symbols()
    protos, consts, _ = _lib.parse_header(open(_lib.HEADER).read())
    for s in SYMBOLS:
        assert s in hdr, f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert _lib.SIGNATURES[s] == protos[s], f"signature of {s} not derived from the header"
    assert _lib.DEIG_BF16 == 2 == consts["DEIG_BF16"]
    assert L.deig_version() == 0x000600  # additive entry points
    # sample pointers are const void*: plain c_void_p, no new type rule in the parser
    assert _lib.SIGNATURES["deig_syrk_bf16"][1][0] is ctypes.c_void_p
    assert _lib.SIGNATURES["deig_syrk_bf16"][1][4] is ctypes.c_float
    assert _lib.SIGNATURES["deig_syrk_bf16_workspace"][0] is ctypes.c_size_t


def _syrk(X=PTR, n=64, d=16, ldx=16, S=PTR, lds=16, flags=0, ws=None, ws_bytes=0):
    return _lib.lib().deig_syrk_bf16(X, n, d, ldx, 1.0, S, lds, flags, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(d=12, ldx=16), "d must be a multiple of 8"),
    (dict(ldx=8), "ldx must be >= d"),
    (dict(ldx=20), "ldx must be a multiple of 8"),
    (dict(X=None), "must not be NULL"),
    (dict(S=None), "must not be NULL"),
    (dict(n=0), "n must be >= 1"),
    (dict(flags=_lib.DEIG_SYRK_ACCUMULATE | 1), "unknown flag bits"),
    (dict(flags=2), "unknown flag bits"),
    (dict(X=PTR + 2), "16-byte aligned"),
    (dict(lds=18), "lds must be"),
])
def test_syrk_argument_rules(kw, word):
    assert _syrk(**kw) == _lib.DEIG_EINVAL
    assert word in _lib.last_error(), _lib.last_error()


def test_syrk_short_workspace():
    L = _lib.lib()
    assert _syrk() == _lib.DEIG_EWORKSPACE  # every argument rule holds, no workspace
    assert "workspace" in _lib.last_error()
    least = L.deig_syrk_bf16_workspace(1, 16)
    assert least > 0
    assert _syrk(ws=PTR, ws_bytes=least - 1) == _lib.DEIG_EWORKSPACE
    assert _syrk(flags=_lib.DEIG_SYRK_ACCUMULATE, ws=PTR, ws_bytes=16) == _lib.DEIG_EWORKSPACE


@pytest.mark.parametrize("d", [8, 520, 3072, 8192])
def test_syrk_workspace_monotone_in_n(d):
    L = _lib.lib()
    last = 0
    for n in (1, 2, 63, 64, 65, 1000, 4096, 16359, 16384, 16385, 65536, 1 << 19, 1 << 21):
        w = L.deig_syrk_bf16_workspace(n, d)
        assert w >= last > -1, (n, d, w, last)
        last = w
    assert L.deig_syrk_bf16_workspace(1, d) > 0
    # no fp32 copy: the recommended workspace of a long shard stays below the shard's fp32 size
    assert L.deig_syrk_bf16_workspace(1 << 21, 8192) < (1 << 21) * 8192 * 4 // 8


def test_transform_argument_rules():
    L = _lib.lib()

    def call(n=8, d=16, ldx=16, k=4, ldw=16, ldy=4, X=PTR, W=PTR, Y=PTR):
        return L.deig_pca_transform_bf16(X, n, d, ldx, None, W, k, ldw, Y, ldy, None, None, None, 0,
                                         None)
    # the full text of deig_last_error(), as a build of the commit before csrc/sample_src.hpp
    # reported it
    for kw, msg in [(dict(k=0), "k=0 must be in 1..256"), (dict(k=257, ldy=257), "k=257 must be in 1..256"),
                    (dict(d=12), "d must be a multiple of 8 (got 12)"),
                    (dict(d=12, ldx=8), "d must be a multiple of 8 (got 12)"),  # two rules: d first
                    (dict(ldx=20), "ldx must be >= d and a multiple of 8 elements"),
                    (dict(ldx=8), "ldx must be >= d and a multiple of 8 elements"),
                    (dict(Y=None), "need at least one output (Y, resid, energy)"),
                    (dict(X=None), "X (16-byte aligned) and W must not be NULL"),
                    (dict(X=PTR + 2), "X (16-byte aligned) and W must not be NULL"),
                    (dict(n=0), "n must be >= 1 (got 0)")]:
        assert call(**kw) == _lib.DEIG_EINVAL, kw
        assert _lib.last_error() == "pca_transform_bf16: " + msg
    assert call() == _lib.DEIG_EWORKSPACE
    for k in (1, 64, 256):
        kp = (k + 15) // 16 * 16
        assert L.deig_pca_transform_bf16_workspace(1 << 20, 3072, k) >= 3072 * kp * 4


def _align(x, a):
    return (x + a - 1) // a * a


# the packed W image (dpad x kp floats) and the padded mean (dpad doubles), each a 256-byte
# aligned slice, dpad = d rounded up to a super-chunk of 64 features
@pytest.mark.parametrize("n,d,k,want", [(1, 8, 1, 4608), (1000, 264, 17, 43520),
                                        (1 << 20, 3072, 256, 3170304)])
def test_transform_workspace_is_exact(n, d, k, want):
    L = _lib.lib()
    dpad, kp = _align(d, 64), _align(k, 16)
    assert want == _align(dpad * kp * 4, 256) + _align(dpad * 8, 256)
    assert L.deig_pca_transform_bf16_workspace(n, d, k) == want
    assert L.deig_pca_transform_bf16_workspace(n, d, 0) == 0
    assert L.deig_pca_transform_bf16_workspace(n, d, 257) == 0


def test_column_passes_know_bf16_and_reject_unknown_types():
    L = _lib.lib()
    # an odd address is misaligned for every type; bf16 needs 2 bytes only
    assert L.deig_colsum(PTR + 2, _lib.DEIG_BF16, 8, 16, 16, PTR, None, 0, None) == _lib.DEIG_EWORKSPACE
    assert L.deig_colsum(PTR + 2, _lib.DEIG_F32, 8, 16, 16, PTR, None, 0, None) == _lib.DEIG_EINVAL
    assert L.deig_colsum(PTR + 1, _lib.DEIG_BF16, 8, 16, 16, PTR, None, 0, None) == _lib.DEIG_EINVAL
    assert L.deig_colsum(PTR, 7, 8, 16, 16, PTR, None, 0, None) == _lib.DEIG_EINVAL
    assert "unknown element type 7" in _lib.last_error(), _lib.last_error()
    assert L.deig_syrk_shift(PTR, 7, 8, 16, 16, 1.0, PTR, 16, None, 16, None, 0, None) == _lib.DEIG_EINVAL
    assert "unknown element type 7" in _lib.last_error(), _lib.last_error()
    assert L.deig_syrk_centered(PTR, 7, 8, 16, 16, None, 1.0, PTR, 16, None, 16, None, None, 0,
                                None) == _lib.DEIG_EINVAL
    assert "unknown element type 7" in _lib.last_error(), _lib.last_error()
    for q in (L.deig_syrk_shift_workspace, L.deig_syrk_centered_workspace):
        assert q(1000, 264, _lib.DEIG_BF16) == q(1000, 264, _lib.DEIG_F32) > 0
