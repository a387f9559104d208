"""C ABI of deig_oja_steps_bf16 (Oja steps on bf16 samples as they are): declared, exported,
bound from the header, bad arguments rejected with a message naming the rule and a short or
NULL workspace reported, all before any GPU work (CPU)."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

PTR = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced


def test_symbol_declared_exported_and_bound():
    L = _lib.lib()
    protos, _, _ = _lib.parse_header(open(_lib.HEADER).read())
    s = "deig_oja_steps_bf16"
    assert s in _lib.header_symbols(), f"include/deig.h does not declare {s}"
    assert hasattr(L, s), f"libdeig.so does not export {s}"
    assert _lib.SIGNATURES[s] == protos[s], f"signature of {s} not derived from the header"
    restype, argtypes = _lib.SIGNATURES[s]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert argtypes[0] is ctypes.c_void_p and argtypes[5] is ctypes.c_float
    assert L.deig_version() == 0x000600  # an additive entry point


def _oja(X=PTR, nb=2, b=64, d=16, ldx=16, V=PTR, k=4, ldv=16, orth_every=1, ws=None, ws_bytes=0):
    return _lib.lib().deig_oja_steps_bf16(X, nb, b, d, ldx, 0.02, V, k, ldv, orth_every, ws,
                                          ws_bytes, None)


# (arguments, the rule's words, the full text of deig_last_error() as a build of the commit
# before csrc/sample_src.hpp reported it)
RULES = [
    (dict(d=12, ldx=16, ldv=16), "d must be a multiple of 8",
     "oja_bf16: d must be a multiple of 8, at least 8 (got 12)"),
    (dict(ldx=8), "ldx must be >= d",
     "oja_bf16: ldx must be >= d"),
    (dict(ldx=20), "ldx must be a multiple of 8",
     "oja_bf16: ldx must be a multiple of 8 elements"),
    (dict(X=None), "must not be NULL",
     "oja_bf16: X and V must not be NULL"),
    (dict(V=None), "must not be NULL",
     "oja_bf16: X and V must not be NULL"),
    (dict(X=PTR + 2), "16-byte aligned",
     "oja_bf16: X must be 16-byte aligned"),
    (dict(k=0), "1 <= k <= min(64, d)",
     "oja_bf16: need 1 <= k <= min(64, d) (got k=0, d=16)"),
    (dict(k=65, d=128, ldx=128, ldv=128), "1 <= k <= min(64, d)",
     "oja_bf16: need 1 <= k <= min(64, d) (got k=65, d=128)"),
    (dict(k=17), "1 <= k <= min(64, d)",
     "oja_bf16: need 1 <= k <= min(64, d) (got k=17, d=16)"),
    (dict(nb=0), "nb must be >= 1",
     "oja_bf16: nb must be >= 1 (got 0)"),
    (dict(b=0), "b must be >= 1",
     "oja_bf16: b must be >= 1 (got 0)"),
    (dict(orth_every=0), "orth_every must be >= 1",
     "oja_bf16: orth_every must be >= 1 (got 0)"),
    (dict(ldv=8), "ldv must be >= d",
     "oja_bf16: ldv must be >= d"),
    # two rules broken at once: d is tested first
    (dict(d=12, ldx=8), "d must be a multiple of 8",
     "oja_bf16: d must be a multiple of 8, at least 8 (got 12)"),
]


def _ids(rules):
    """pytest's own ids of these tables when they held (arguments, word) pairs: kept, so that
    every case keeps its name."""
    return [f"kw{i}-{word}" for i, (_, word, _) in enumerate(rules)]


@pytest.mark.parametrize("kw,word,msg", RULES, ids=_ids(RULES))
def test_argument_rules(kw, word, msg):
    assert _oja(**kw) == _lib.DEIG_EINVAL
    assert word in msg and _lib.last_error() == msg


def test_short_or_null_workspace():
    L = _lib.lib()
    assert _oja() == _lib.DEIG_EWORKSPACE  # every argument rule holds, no workspace
    assert "workspace" in _lib.last_error()
    need = L.deig_oja_workspace(64, 16, 4)
    assert need > 0
    assert _oja(ws=PTR, ws_bytes=need - 1) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _oja(ws=None, ws_bytes=need) == _lib.DEIG_EWORKSPACE
