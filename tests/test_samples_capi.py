"""C ABI of the covariance-free worker route - deig_gram_apply, deig_topk_samples and their
workspace queries - and the constructor validation of the Python routes built on it: declared,
exported, bound from the header, bad arguments rejected with a message naming the rule and a
short or NULL workspace reported, all before any GPU work (CPU)."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

PTR = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced
F32, F64, BF16, U8 = 0, 1, 2, 3
SYMBOLS = {"deig_gram_apply": (ctypes.c_int, 15), "deig_gram_apply_workspace": (ctypes.c_size_t, 4),
           "deig_topk_samples": (ctypes.c_int, 23), "deig_topk_samples_workspace": (ctypes.c_size_t, 6)}


def test_symbols_bound_from_the_header():
    L = _lib.lib()
    protos, consts, _ = _lib.parse_header(open(_lib.HEADER).read())
    for s, (res, nargs) in SYMBOLS.items():
        assert s in _lib.header_symbols(), f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert _lib.SIGNATURES[s] == protos[s], f"signature of {s} not derived from the header"
        restype, argtypes = _lib.SIGNATURES[s]
        assert restype is res and len(argtypes) == nargs
    args = _lib.SIGNATURES["deig_gram_apply"][1]
    assert args[1] is ctypes.c_int and args[5] is ctypes.c_void_p and args[6] is ctypes.c_float
    assert _lib.SIGNATURES["deig_topk_samples"][1][19] == ctypes.POINTER(_lib.SolverOpts)
    assert consts["DEIG_U8"] == U8
    assert L.deig_version() == 0x000600  # additive entry points


def _gram(xtype=F32, X=PTR, n=10, d=32, ldx=32, center=PTR, Q=PTR, p=16, ldq=16, Y=PTR, ldy=16,
          ws=None, ws_bytes=0):
    return _lib.lib().deig_gram_apply(X, xtype, n, d, ldx, center, 0.1, Q, p, ldq, Y, ldy, ws, ws_bytes,
                                      None)


def _topk(xtype=F32, X=PTR, n=10, d=32, ldx=32, center=PTR, k=4, p=16, max_sweeps=10, Q0=None, k0=0,
          ldq0=32, V=PTR, ldv=32, evals=PTR, ws=None, ws_bytes=0):
    sweeps, resid = ctypes.c_int(0), ctypes.c_float(0)
    return _lib.lib().deig_topk_samples(X, xtype, n, d, ldx, center, 0.1, k, p, max_sweeps, 1e-6, Q0, k0,
                                        ldq0, V, ldv, evals, ctypes.byref(sweeps), ctypes.byref(resid),
                                        None, ws, ws_bytes, None)


# (arguments, the rule's words, the full text of deig_last_error() behind the entry point's name
# as a build of the commit before csrc/sample_src.hpp reported it); SAMPLE_RULES and TWO_RULES
# are gram_apply_check's, which both entry points run first
SAMPLE_RULES = [
    (dict(xtype=F64), "xtype must be",
     "xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got 1)"),
    (dict(xtype=7), "xtype must be",
     "xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got 7)"),
    (dict(xtype=F32, d=30), "d must be a multiple of 4",
     "d must be a multiple of 4 (got 30)"),
    (dict(xtype=U8, d=30), "d must be a multiple of 4",
     "d must be a multiple of 4 (got 30)"),
    (dict(xtype=BF16, d=28), "d must be a multiple of 8",
     "d must be a multiple of 8 (got 28)"),
    (dict(xtype=F32, ldx=28), "ldx must be >= d",
     "ldx must be >= d"),
    (dict(xtype=BF16, ldx=24), "ldx must be >= d",
     "ldx must be >= d"),
    (dict(xtype=U8, ldx=28), "ldx must be >= d",
     "ldx must be >= d"),
    (dict(xtype=F32, ldx=34), "ldx must be a multiple of 4",
     "ldx must be a multiple of 4 elements"),
    (dict(xtype=U8, ldx=34), "ldx must be a multiple of 4",
     "ldx must be a multiple of 4 elements"),
    (dict(xtype=BF16, ldx=36), "ldx must be a multiple of 8",
     "ldx must be a multiple of 8 elements"),
    (dict(d=12, ldx=12), "d must be >= 16",
     "d must be >= 16 (got 12)"),
    (dict(n=0), "n must be >= 1",
     "n must be >= 1 (got 0)"),
    (dict(X=None), "must not be NULL",
     "X must not be NULL"),
    (dict(xtype=F32, X=PTR + 4), "16-byte aligned",
     "X must be 16-byte aligned"),
    (dict(xtype=BF16, X=PTR + 2), "16-byte aligned",
     "X must be 16-byte aligned"),
    (dict(xtype=U8, X=PTR + 2), "4-byte aligned",
     "X must be 4-byte aligned"),
    (dict(center=PTR + 4), "center must be aligned",
     "center must be aligned to its element size"),
]


GRAM_RULES = [
    (dict(p=24, ldq=24, ldy=24), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 24)"),
    (dict(p=0), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 0)"),
    (dict(p=144, d=256, ldx=256, ldq=144, ldy=144), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 144)"),
    (dict(Q=None), "must not be NULL",
     "Q and Y must not be NULL"),
    (dict(Y=None), "must not be NULL",
     "Q and Y must not be NULL"),
    (dict(Q=PTR + 4), "16-byte aligned",
     "Q and Y must be 16-byte aligned"),
    (dict(Y=PTR + 8), "16-byte aligned",
     "Q and Y must be 16-byte aligned"),
    (dict(ldq=12), "ldq must be >= p",
     "ldq must be >= p and a multiple of 4"),
    (dict(ldq=18), "ldq must be >= p and a multiple of 4",
     "ldq must be >= p and a multiple of 4"),
    (dict(ldy=12), "ldy must be >= p",
     "ldy must be >= p and a multiple of 4"),
    (dict(ldy=18), "ldy must be >= p and a multiple of 4",
     "ldy must be >= p and a multiple of 4"),
]
TOPK_RULES = [
    (dict(k=0), "1 <= k <= min(128, d)",
     "need 1 <= k <= min(128, d) (k=0, d=32)"),
    (dict(k=33, p=48), "1 <= k <= min(128, d)",
     "need 1 <= k <= min(128, d) (k=33, d=32)"),
    (dict(k=129, p=128, d=256, ldx=256, ldv=256), "1 <= k <= min(128, d)",
     "need 1 <= k <= min(128, d) (k=129, d=256)"),
    (dict(p=24), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 24)"),
    (dict(p=0), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 0)"),
    (dict(p=144, d=256, ldx=256, ldv=256), "p must be a multiple of 16",
     "p must be a multiple of 16 in 16..128 (got 144)"),
    (dict(k=20, p=16), "k <= p <= d",
     "the subspace needs k <= p <= d (k=20, p=16, d=32)"),
    (dict(p=48), "k <= p <= d",
     "the subspace needs k <= p <= d (k=4, p=48, d=32)"),
    (dict(V=None), "must not be NULL",
     "V and evals must not be NULL, ldv >= d"),
    (dict(evals=None), "must not be NULL",
     "V and evals must not be NULL, ldv >= d"),
    (dict(ldv=16), "ldv >= d",
     "V and evals must not be NULL, ldv >= d"),
    (dict(max_sweeps=0), "max_sweeps must be >= 1",
     "max_sweeps must be >= 1"),
    (dict(k0=2, Q0=None), "warm start",
     "bad warm start (k0=2, p=16)"),
]
TWO_RULES = [  # two rules broken at once: d is tested first
    (dict(xtype=F32, d=30, ldx=28), "d must be a multiple of 4", "d must be a multiple of 4 (got 30)"),
    (dict(xtype=U8, d=30, ldx=28), "d must be a multiple of 4", "d must be a multiple of 4 (got 30)"),
    (dict(xtype=BF16, d=28, ldx=24), "d must be a multiple of 8", "d must be a multiple of 8 (got 28)"),
]


def _ids(rules):
    """pytest's own ids of these tables when they held (arguments, word) pairs: kept, so that
    every case keeps its name."""
    return [f"kw{i}-{word}" for i, (_, word, _) in enumerate(rules)]


@pytest.mark.parametrize("kw,word,msg", SAMPLE_RULES + GRAM_RULES + TWO_RULES,
                         ids=_ids(SAMPLE_RULES + GRAM_RULES + TWO_RULES))
def test_gram_apply_argument_rules(kw, word, msg):
    assert _gram(**kw) == _lib.DEIG_EINVAL
    assert word in msg and _lib.last_error() == "gram_apply: " + msg


@pytest.mark.parametrize("kw,word,msg", SAMPLE_RULES + TOPK_RULES + TWO_RULES,
                         ids=_ids(SAMPLE_RULES + TOPK_RULES + TWO_RULES))
def test_topk_samples_argument_rules(kw, word, msg):
    assert _topk(**kw) == _lib.DEIG_EINVAL
    assert word in msg and _lib.last_error() == "topk_samples: " + msg


@pytest.mark.parametrize("xtype", [F32, BF16, U8])
@pytest.mark.parametrize("center", [PTR, None])
def test_short_or_null_workspace(xtype, center):
    L = _lib.lib()
    X = PTR + 4 if xtype == U8 else PTR
    # the operator: any workspace of at least query(n', ...) bytes, 1 <= n' <= n, is accepted
    assert _gram(xtype=xtype, X=X, center=center) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    least = L.deig_gram_apply_workspace(1, 32, 16, xtype)
    assert 0 < least <= L.deig_gram_apply_workspace(10, 32, 16, xtype)
    assert _gram(xtype=xtype, X=X, center=center, ws=PTR, ws_bytes=least - 1) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _gram(xtype=xtype, X=X, center=center, ws=None, ws_bytes=least) == _lib.DEIG_EWORKSPACE
    # the solve
    need = L.deig_topk_samples_workspace(10, 32, 4, 16, xtype, None)
    assert need > 0
    assert _topk(xtype=xtype, X=X, center=center) == _lib.DEIG_EWORKSPACE
    assert _topk(xtype=xtype, X=X, center=center, ws=PTR, ws_bytes=need - 1) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _topk(xtype=xtype, X=X, center=center, ws=None, ws_bytes=need) == _lib.DEIG_EWORKSPACE


@pytest.mark.parametrize("xtype", [F32, BF16, U8])
def test_workspace_queries(xtype):
    L = _lib.lib()
    ns = (1, 2, 31, 32, 33, 64, 255, 256, 257, 1000, 4096, 65536, 1 << 20)
    for d in (16, 136, 3072, 40960):
        for p in (16, 48, 128):
            if p > d:
                continue
            g = [L.deig_gram_apply_workspace(n, d, p, xtype) for n in ns]
            t = [L.deig_topk_samples_workspace(n, d, min(p, 10), p, xtype, None) for n in ns]
            assert all(v > 0 for v in g + t)
            assert g == sorted(g) and t == sorted(t), (d, p)
        for n in (5, 3000):
            ps = [p for p in range(16, 129, 16) if p <= d]
            g = [L.deig_gram_apply_workspace(n, d, p, xtype) for p in ps]
            t = [L.deig_topk_samples_workspace(n, d, 8, p, xtype, None) for p in ps]
            assert g == sorted(g) and t == sorted(t), (d, n)
    # shapes the launches reject
    q = 8 if xtype == BF16 else 4
    for args in ((0, 32, 16), (10, 12, 16), (10, 32 + q // 2, 16), (10, 32, 24), (10, 32, 0), (10, 256, 144)):
        assert L.deig_gram_apply_workspace(*args, xtype) == 0, args
    for args in ((0, 32, 4, 16), (10, 12, 4, 16), (10, 32, 0, 16), (10, 32, 20, 16), (10, 32, 4, 48),
                 (10, 32, 4, 24), (10, 256, 129, 128)):
        assert L.deig_topk_samples_workspace(*args, xtype, None) == 0, args
    assert L.deig_gram_apply_workspace(10, 32, 16, F64) == 0
    assert L.deig_topk_samples_workspace(10, 32, 4, 16, 7, None) == 0


def test_estimator_and_pca_constructor_validation():
    from distributed_eigenspaces_amd.estimator import DistributedEigenspaceEstimator
    from distributed_eigenspaces_amd.pca import PCA
    with pytest.raises(ValueError, match="covariance must be one of"):
        DistributedEigenspaceEstimator(4, covariance="nope")
    with pytest.raises(ValueError, match="covariance must be one of"):
        PCA(4, covariance="nope")
    with pytest.raises(ValueError, match="raw bytes only"):
        DistributedEigenspaceEstimator(4, center=True, u8_mode="gray", covariance="free")
    with pytest.raises(ValueError, match="raw bytes only"):
        PCA(4, u8_mode="gray", covariance="free")
    e = DistributedEigenspaceEstimator(4, workers_per_rank=4, concurrent_workers=True, covariance="free")
    assert e.covariance == "free" and not e.batched and not e.concurrent  # the serial worker loop
    assert DistributedEigenspaceEstimator(4).covariance == "explicit"
    assert PCA(4).covariance == "explicit" and PCA(4, covariance="free", u8_mode="raw").covariance == "free"
