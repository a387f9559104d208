"""C ABI of the wide-data worker route - deig_gram_outer, deig_topk_dual and their workspace
queries - and the validation of the Python routes built on it: declared, exported, bound from
the header, bad arguments rejected with a message naming the rule and a short or NULL
workspace reported, all before any GPU work (CPU)."""
import ctypes

import pytest
import torch

from distributed_eigenspaces_amd import _lib

PTR = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced
F32, F64, BF16, U8 = 0, 1, 2, 3
SYMBOLS = {"deig_gram_outer": (ctypes.c_int, 13), "deig_gram_outer_workspace": (ctypes.c_size_t, 4),
           "deig_topk_dual": (ctypes.c_int, 20), "deig_topk_dual_workspace": (ctypes.c_size_t, 6)}


def test_symbols_bound_from_the_header():
    L = _lib.lib()
    protos, _, _ = _lib.parse_header(open(_lib.HEADER).read())
    for s, (res, nargs) in SYMBOLS.items():
        assert s in _lib.header_symbols(), f"include/deig.h does not declare {s}"
        assert hasattr(L, s), f"libdeig.so does not export {s}"
        assert _lib.SIGNATURES[s] == protos[s], f"signature of {s} not derived from the header"
        restype, argtypes = _lib.SIGNATURES[s]
        assert restype is res and len(argtypes) == nargs
    assert _lib.SIGNATURES["deig_topk_dual"][1][16] == ctypes.POINTER(_lib.SolverOpts)
    assert L.deig_version() == 0x000600  # additive entry points


def _outer(xtype=F32, X=PTR, n=10, d=32, ldx=32, center=PTR, K=PTR, ldk=12, flags=0, ws=None, ws_bytes=0):
    return _lib.lib().deig_gram_outer(X, xtype, n, d, ldx, center, 0.1, K, ldk, flags, ws, ws_bytes, None)


def _dual(xtype=F32, X=PTR, n=10, d=32, ldx=32, center=PTR, k=4, p=16, max_sweeps=10, V=PTR, ldv=32,
          evals=PTR, ws=None, ws_bytes=0):
    sweeps, resid = ctypes.c_int(0), ctypes.c_float(0)
    return _lib.lib().deig_topk_dual(X, xtype, n, d, ldx, center, 0.1, k, p, max_sweeps, 1e-6, V, ldv,
                                     evals, ctypes.byref(sweeps), ctypes.byref(resid), None, ws, ws_bytes,
                                     None)


# the rules both entry points take from deig_gram_apply (gram_apply_check)
SAMPLE_RULES = [
    (dict(xtype=F64), "xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got 1)"),
    (dict(xtype=F32, d=30), "d must be a multiple of 4 (got 30)"),
    (dict(xtype=BF16, d=28), "d must be a multiple of 8 (got 28)"),
    (dict(xtype=U8, ldx=34), "ldx must be a multiple of 4 elements"),
    (dict(ldx=28), "ldx must be >= d"),
    (dict(n=0), "n must be >= 1 (got 0)"),
    (dict(X=None), "X must not be NULL"),
    (dict(xtype=F32, X=PTR + 4), "X must be 16-byte aligned"),
    (dict(xtype=BF16, X=PTR + 2), "X must be 16-byte aligned"),
    (dict(xtype=U8, X=PTR + 2), "X must be 4-byte aligned"),
    (dict(center=PTR + 4), "center must be aligned to its element size"),
]
OUTER_RULES = [
    (dict(flags=1), "flags must be 0 (got 0x1)"),
    (dict(flags=0x100), "flags must be 0 (got 0x100)"),
    (dict(n=32769, ldk=32772), "n must be <= 32768 (got 32769)"),
    (dict(K=None), "K must not be NULL"),
    (dict(K=PTR + 4), "K must be 16-byte aligned"),
    (dict(ldk=8), "ldk must be >= n"),
    (dict(ldk=14), "ldk must be a multiple of 4"),
]
DUAL_RULES = [
    (dict(n=32769), "n must be <= 32768 (got 32769): the n x n Gram matrix is the route for n <= d; "
                    "use deig_topk_samples"),
    (dict(k=0), "need 1 <= k <= min(128, n, d) (k=0, n=10, d=32)"),
    (dict(k=11), "need 1 <= k <= min(128, n, d) (k=11, n=10, d=32)"),
    (dict(k=33, n=64, p=48), "need 1 <= k <= min(128, n, d) (k=33, n=64, d=32)"),
    (dict(k=129, p=128, n=200, d=256, ldx=256, ldv=256), "need 1 <= k <= min(128, n, d) (k=129, n=200, d=256)"),
    (dict(p=24), "p must be a multiple of 16 in 16..128 (got 24)"),
    (dict(p=48), "the subspace needs k <= p <= d (k=4, p=48, d=32)"),
    (dict(max_sweeps=0), "max_sweeps must be >= 1"),
    (dict(V=None), "V and evals must not be NULL, ldv >= d"),
    (dict(ldv=16), "V and evals must not be NULL, ldv >= d"),
]


@pytest.mark.parametrize("kw,msg", SAMPLE_RULES + OUTER_RULES)
def test_gram_outer_argument_rules(kw, msg):
    assert _outer(**kw) == _lib.DEIG_EINVAL
    assert _lib.last_error() == "gram_outer: " + msg


@pytest.mark.parametrize("kw,msg", SAMPLE_RULES + DUAL_RULES)
def test_topk_dual_argument_rules(kw, msg):
    assert _dual(**kw) == _lib.DEIG_EINVAL
    assert _lib.last_error() == "topk_dual: " + msg


@pytest.mark.parametrize("xtype", [F32, BF16, U8])
@pytest.mark.parametrize("center", [PTR, None])
def test_short_or_null_workspace(xtype, center):
    L = _lib.lib()
    X = PTR + 4 if xtype == U8 else PTR
    least = L.deig_gram_outer_workspace(10, 16, xtype, int(center is not None))
    assert 0 < least <= L.deig_gram_outer_workspace(10, 32, xtype, int(center is not None))
    assert _outer(xtype=xtype, X=X, center=center) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _outer(xtype=xtype, X=X, center=center, ws=PTR, ws_bytes=least - 1) == _lib.DEIG_EWORKSPACE
    assert _outer(xtype=xtype, X=X, center=center, ws=None, ws_bytes=least) == _lib.DEIG_EWORKSPACE
    need = L.deig_topk_dual_workspace(10, 32, 4, 16, xtype, None)
    assert need > 0
    assert _dual(xtype=xtype, X=X, center=center) == _lib.DEIG_EWORKSPACE
    assert _dual(xtype=xtype, X=X, center=center, ws=PTR, ws_bytes=need - 1) == _lib.DEIG_EWORKSPACE
    assert "workspace" in _lib.last_error()
    assert _dual(xtype=xtype, X=X, center=center, ws=None, ws_bytes=need) == _lib.DEIG_EWORKSPACE


@pytest.mark.parametrize("xtype", [F32, BF16, U8])
def test_workspace_queries(xtype):
    L = _lib.lib()
    ds = (16, 64, 72, 136, 1032, 3072, 16384, 16424, 32768, 40960, 65536, 1 << 20)
    for n in (1, 50, 128, 129, 384, 1024, 4096, 8192, 32768):
        for centred in (0, 1):
            g = [L.deig_gram_outer_workspace(n, d, xtype, centred) for d in ds]
            assert all(v > 0 for v in g) and g == sorted(g), (n, centred)
        assert L.deig_gram_outer_workspace(n, 136, xtype, 0) <= L.deig_gram_outer_workspace(n, 136, xtype, 1)
        for k, p in ((1, 16), (10, 16), (100, 128)):
            if k > n:
                continue
            t = [L.deig_topk_dual_workspace(n, d, k, p, xtype, None) for d in ds if d >= p]
            assert all(v > 0 for v in t) and t == sorted(t), (n, k, p)
    # shapes the launches reject
    q = 8 if xtype == BF16 else 4
    for args in ((0, 32), (32769, 32), (10, 12), (10, 32 + q // 2)):
        assert L.deig_gram_outer_workspace(*args, xtype, 0) == 0, args
    for args in ((0, 32, 4, 16), (32769, 32, 4, 16), (10, 32 + q // 2, 4, 16), (10, 32, 0, 16), (10, 32, 11, 16),
                 (10, 32, 4, 24), (10, 32, 4, 48), (200, 256, 129, 128)):
        assert L.deig_topk_dual_workspace(*args, xtype, None) == 0, args
    assert L.deig_gram_outer_workspace(10, 32, F64, 0) == 0
    assert L.deig_topk_dual_workspace(10, 32, 4, 16, F64, None) == 0


def test_python_routes_validate():
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd.estimator import COVARIANCES, DistributedEigenspaceEstimator
    from distributed_eigenspaces_amd.pca import PCA
    assert COVARIANCES == ("explicit", "free", "dual")
    e = DistributedEigenspaceEstimator(4, workers_per_rank=4, concurrent_workers=True, covariance="dual")
    assert e.covariance == "dual" and not e.batched and not e.concurrent  # the serial worker loop
    assert PCA(4, covariance="dual", u8_mode="raw").covariance == "dual"
    with pytest.raises(ValueError, match="covariance='dual' reads uint8 samples as raw bytes only"):
        DistributedEigenspaceEstimator(4, center=True, u8_mode="gray", covariance="dual")
    with pytest.raises(ValueError, match="covariance='dual' reads uint8 samples as raw bytes only"):
        PCA(4, u8_mode="gray", covariance="dual")
    with pytest.raises(TypeError, match="float64 samples are not supported"):
        de.topk_dual(torch.zeros((8, 32), dtype=torch.float64), 2)
    with pytest.raises(TypeError, match="float64 samples are not supported"):
        de.gram_outer(torch.zeros((8, 32), dtype=torch.float64))
    with pytest.raises(ValueError, match="exceeds the n=8 rows"):
        de.topk_dual(torch.zeros((8, 32), dtype=torch.float32), 9)
    assert de.topk_dual is de.linalg.topk_dual and de.gram_outer is de.linalg.gram_outer
