"""C ABI of deig_oja_steps_centered (Oja steps about a centre on float32, bf16 and uint8
samples as they are): declared, exported, bound from the header with DEIG_U8, bad arguments
rejected with a message naming the rule and a short or NULL workspace reported, all before any
GPU work (CPU)."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

PTR = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced
F32, F64, BF16, U8 = 0, 1, 2, 3


def test_symbol_and_element_type_bound_from_the_header():
    L = _lib.lib()
    protos, consts, _ = _lib.parse_header(open(_lib.HEADER).read())
    s = "deig_oja_steps_centered"
    assert s in _lib.header_symbols(), f"include/deig.h does not declare {s}"
    assert hasattr(L, s), f"libdeig.so does not export {s}"
    assert _lib.SIGNATURES[s] == protos[s], f"signature of {s} not derived from the header"
    restype, argtypes = _lib.SIGNATURES[s]
    assert restype is ctypes.c_int and len(argtypes) == 15
    assert argtypes[0] is ctypes.c_void_p and argtypes[1] is ctypes.c_int
    assert argtypes[6] is ctypes.c_void_p and argtypes[7] is ctypes.c_float
    assert consts["DEIG_U8"] == 3 and _lib.DEIG_U8 == 3
    assert (_lib.DEIG_F32, _lib.DEIG_F64, _lib.DEIG_BF16) == (F32, F64, BF16)
    assert L.deig_version() == 0x000600  # an additive entry point


def _oja(xtype=F32, X=PTR, nb=2, b=64, d=16, ldx=16, center=PTR, V=PTR, k=4, ldv=16, orth_every=1,
         ws=None, ws_bytes=0):
    return _lib.lib().deig_oja_steps_centered(X, xtype, nb, b, d, ldx, center, 0.02, V, k, ldv,
                                              orth_every, ws, ws_bytes, None)


# (arguments, the rule's words, the full text of deig_last_error() as a build of the commit
# before csrc/sample_src.hpp reported it)
RULES = [
    (dict(xtype=F64), "xtype must be",
     "oja_centered: xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got 1)"),
    (dict(xtype=7), "xtype must be",
     "oja_centered: xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got 7)"),
    (dict(xtype=F32, d=14), "d must be a multiple of 4",
     "oja_centered: d must be a multiple of 4, at least 4 (got 14)"),
    (dict(xtype=U8, d=14), "d must be a multiple of 4",
     "oja_centered: d must be a multiple of 4, at least 4 (got 14)"),
    (dict(xtype=BF16, d=12), "d must be a multiple of 8",
     "oja_centered: d must be a multiple of 8, at least 8 (got 12)"),
    (dict(xtype=F32, ldx=12), "ldx must be >= d",
     "oja_centered: ldx must be >= d"),
    (dict(xtype=BF16, ldx=8), "ldx must be >= d",
     "oja_centered: ldx must be >= d"),
    (dict(xtype=U8, ldx=12), "ldx must be >= d",
     "oja_centered: ldx must be >= d"),
    (dict(xtype=F32, ldx=18), "ldx must be a multiple of 4",
     "oja_centered: ldx must be a multiple of 4 elements"),
    (dict(xtype=U8, ldx=18), "ldx must be a multiple of 4",
     "oja_centered: ldx must be a multiple of 4 elements"),
    (dict(xtype=BF16, ldx=20), "ldx must be a multiple of 8",
     "oja_centered: ldx must be a multiple of 8 elements"),
    (dict(k=0), "1 <= k <= min(64, d)",
     "oja_centered: need 1 <= k <= min(64, d) (got k=0, d=16)"),
    (dict(k=65, d=128, ldx=128, ldv=128), "1 <= k <= min(64, d)",
     "oja_centered: need 1 <= k <= min(64, d) (got k=65, d=128)"),
    (dict(k=17), "1 <= k <= min(64, d)",
     "oja_centered: need 1 <= k <= min(64, d) (got k=17, d=16)"),
    (dict(orth_every=0), "orth_every must be >= 1",
     "oja_centered: orth_every must be >= 1 (got 0)"),
    (dict(nb=0), "nb must be >= 1",
     "oja_centered: nb must be >= 1 (got 0)"),
    (dict(b=0), "b must be >= 1",
     "oja_centered: b must be >= 1 (got 0)"),
    (dict(ldv=8), "ldv must be >= d",
     "oja_centered: ldv must be >= d"),
    (dict(X=None), "must not be NULL",
     "oja_centered: X and V must not be NULL"),
    (dict(V=None), "must not be NULL",
     "oja_centered: X and V must not be NULL"),
    (dict(xtype=F32, X=PTR + 4), "16-byte aligned",
     "oja_centered: X must be 16-byte aligned"),
    (dict(xtype=BF16, X=PTR + 2), "16-byte aligned",
     "oja_centered: X must be 16-byte aligned"),
    (dict(xtype=U8, X=PTR + 2), "4-byte aligned",
     "oja_centered: X must be 4-byte aligned"),
    (dict(center=PTR + 4), "center must be aligned",
     "oja_centered: center must be aligned to its element size"),
    # two rules broken at once: d is tested first
    (dict(xtype=F32, d=14, ldx=12), "d must be a multiple of 4",
     "oja_centered: d must be a multiple of 4, at least 4 (got 14)"),
    (dict(xtype=U8, d=14, ldx=12), "d must be a multiple of 4",
     "oja_centered: d must be a multiple of 4, at least 4 (got 14)"),
    (dict(xtype=BF16, d=12, ldx=8), "d must be a multiple of 8",
     "oja_centered: d must be a multiple of 8, at least 8 (got 12)"),
]


def _ids(rules):
    """pytest's own ids of these tables when they held (arguments, word) pairs: kept, so that
    every case keeps its name."""
    return [f"kw{i}-{word}" for i, (_, word, _) in enumerate(rules)]


@pytest.mark.parametrize("kw,word,msg", RULES, ids=_ids(RULES))
def test_argument_rules(kw, word, msg):
    assert _oja(**kw) == _lib.DEIG_EINVAL
    assert word in msg and _lib.last_error() == msg


@pytest.mark.parametrize("xtype", [F32, BF16, U8])
@pytest.mark.parametrize("center", [PTR, None])
def test_short_or_null_workspace(xtype, center):
    L = _lib.lib()
    # every argument rule holds (uint8: 4-byte alignment is enough; no centre is allowed)
    X = PTR + 4 if xtype == U8 else PTR
    assert _oja(xtype=xtype, X=X, center=center) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    need = L.deig_oja_workspace(64, 16, 4)
    assert need > 0
    assert _oja(xtype=xtype, X=X, center=center, ws=PTR, ws_bytes=need - 1) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _oja(xtype=xtype, X=X, center=center, ws=None, ws_bytes=need) == _lib.DEIG_EWORKSPACE
