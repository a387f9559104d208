"""The skinny fp32-MFMA GEMM (linalg.gemm_skinny / deig_gemm_skinny_f32) and the
projection (linalg.project / deig_project_f32) against float64 numpy of the same
operation, at the smallest shapes that reach every path of csrc/skinny.hip:

* all 16 N instantiations of both forms, M tails, K tails, split-K with uneven slices
  (K = 520: 17 chunks in 2 slices; K = 1100: 35 chunks in 4), both reduce kernels
  (float4: C 16-byte aligned with ldc % 4 == 0; scalar otherwise), alpha / beta;
* integer data: every partial sum is an integer below 2^24, so the result must equal the
  float64 reference bit for bit whatever the slicing or summation order;
* real data: the worst-case bound of a length-K fp32 dot product in any order,
  |C - C_ref| <= (K + 8) 2^-23 (|alpha| |op(A)| |B| + |beta| |C0|), derived, not measured
  (2^-23 covers truncating as well as rounding adds inside the MFMA);
* operands are views into larger allocations: NaN in the padding of A and B, a sentinel in
  C's padding and in three rows below it (bit-unchanged afterwards), the cached workspace
  filled with 0xFF bytes first.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from distributed_eigenspaces_amd import _lib, linalg

pytestmark = pytest.mark.gpu

SENT = np.float32(-777.125)  # in the padding of C / Y
EPS = 2.0 ** -23
POISON_BYTES = 64 << 20

ALL_N = list(range(16, 257, 16))
M_TAILS = {False: [1, 63, 65, 77], True: [4, 60, 68]}        # (N): M free; (T): M % 4 == 0
K_SINGLE = {False: [4, 36, 100], True: [1, 3, 33, 100]}      # (N): K % 4 == 0; (T): K free
K_SPLIT = [520, 1100]
C_MODES = ["contig", "pad4", "pad1", "off1"]  # float4 reduce: contig, pad4; scalar: pad1, off1
ALPHA_BETA = [(1.0, 0.0), (0.5, 0.0), (-2.0, 1.0), (1.0, 0.5)]


def expected_slices(K):
    """choose_ks of csrc/skinny.hip for the few row blocks used here (M <= 128), where
    only the cap of 8 chunks per slice binds: 1 below K = 481, 2 at 520, 4 at 1100."""
    return max(((K + 31) // 32) // 8, 1)


def check_split(M, N, K):
    """The workspace query proves that split-K is (in)active where the case means it."""
    ks = expected_slices(K)
    ws = _lib.lib().deig_gemm_skinny_workspace(M, N, K)
    if K in K_SPLIT or K > 512:
        assert ks > 1 and ws > 0, (M, N, K)
        assert ws == ks * M * N * 4, (M, N, K, ws)
    else:
        assert ws == 0, (M, N, K, ws)


def poison_workspace(dev, fill=0xFF):
    linalg._workspace(dev, POISON_BYTES).fill_(fill)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def draw(rng, shape, kind):
    if kind == "int":
        return rng.integers(-4, 5, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def padded_view(a, pad, dev):
    """``a`` as a view into an allocation with ``pad`` more columns, all NaN."""
    big = np.full((a.shape[0], a.shape[1] + pad), np.nan, np.float32)
    big[:, :a.shape[1]] = a
    return torch.from_numpy(big).to(dev)[:, :a.shape[1]]


class Out:
    """An (M, N) output inside a larger sentinel-filled allocation: ``pad`` more columns,
    three more rows, ``off`` floats in front."""

    def __init__(self, M, N, mode, dev, init=None):
        pad, off = {"contig": (0, 0), "pad4": (4, 0), "pad3": (3, 0), "pad1": (1, 0),
                    "off1": (0, 1)}[mode]
        self.M, self.N, self.ld, self.off = M, N, N + pad, off
        host = np.full(off + (M + 3) * self.ld, SENT, np.float32)
        body = host[off:].reshape(M + 3, self.ld)
        body[:M, :N] = np.nan if init is None else init
        self.flat = torch.from_numpy(host).to(dev)
        self.view = self.flat[off:].view(M + 3, self.ld)[:M, :N]
        self.host0 = host

    def read(self):
        """(the M x N result, True if everything around it is bit-unchanged)."""
        got = self.flat.cpu().numpy()
        body = got[self.off:].reshape(self.M + 3, self.ld)
        res = body[:self.M, :self.N].copy()
        body[:self.M, :self.N] = 0
        ref = self.host0.copy()
        ref[self.off:].reshape(self.M + 3, self.ld)[:self.M, :self.N] = 0
        return res, np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def run_gemm(dev, trans, M, N, K, alpha, beta, cmode, kind):
    """One gemm_skinny call on padded views with a poisoned workspace.  Returns the
    result, the float64 reference and the bound's magnitude term."""
    rng = np.random.default_rng(seed_of(trans, M, N, K, alpha, beta, cmode, kind))
    a = draw(rng, (K, M) if trans else (M, K), kind)
    b = draw(rng, (K, N), kind)
    c0 = draw(rng, (M, N), kind)
    A, B = padded_view(a, 4, dev), padded_view(b, 4, dev)
    out = Out(M, N, cmode, dev, init=c0 if beta != 0.0 else None)  # beta == 0: C holds NaN
    check_split(M, N, K)
    poison_workspace(dev)
    C = linalg.gemm_skinny(A, B, trans, alpha, beta, C=out.view)
    assert C is out.view
    res, untouched = out.read()
    assert untouched, "wrote outside C"
    opa = (a.T if trans else a).astype(np.float64)
    b64, c64 = b.astype(np.float64), c0.astype(np.float64)
    ref = alpha * (opa @ b64) + (beta * c64 if beta != 0.0 else 0.0)
    mag = abs(alpha) * (np.abs(opa) @ np.abs(b64)) + abs(beta) * np.abs(c64)
    return res, ref, mag


def exact_grid():
    cases = []
    for trans in (False, True):
        ms, k1 = M_TAILS[trans], K_SINGLE[trans]
        for i, N in enumerate(ALL_N):  # every instantiation, single-slice and split-K
            cases.append((trans, ms[i % len(ms)], N, k1[i % len(k1)]))
            cases.append((trans, ms[(i + 1) % len(ms)], N, K_SPLIT[i % 2]))
        for N in (16, 160):            # every M tail with every K tail
            for M in ms:
                for K in k1 + K_SPLIT:
                    cases.append((trans, M, N, K))
    return sorted(set(cases))


def case_id(c):
    return "-".join(("T" if x else "N") if isinstance(x, bool) else str(x) for x in c)


# ---------------------------------------------------------------- exactness
EXACT_GRID = exact_grid()


@pytest.mark.parametrize("trans,M,N,K", EXACT_GRID, ids=[case_id(c) for c in EXACT_GRID])
def test_integer_data_is_exact(trans, M, N, K, cuda):
    cmode = C_MODES[(M + N // 16 + K) % len(C_MODES)]
    res, ref, _ = run_gemm(cuda, trans, M, N, K, 1.0, 0.0, cmode, "int")
    assert np.isfinite(res).all()
    assert np.array_equal(res.astype(np.float64), ref), (cmode, np.abs(res - ref).max())


EPILOGUE_SHAPES = [(False, 65, 80, 100), (False, 77, 32, 520), (True, 68, 80, 33),
                   (True, 60, 32, 1100)]


@pytest.mark.parametrize("cmode", C_MODES)
@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
@pytest.mark.parametrize("trans,M,N,K", EPILOGUE_SHAPES, ids=[case_id(c) for c in EPILOGUE_SHAPES])
def test_alpha_beta_and_both_epilogues_exact(trans, M, N, K, alpha, beta, cmode, cuda):
    """alpha / beta in the single-slice epilogue and in both reduce kernels; with
    beta == 0 C holds NaN beforehand and must not be read."""
    res, ref, _ = run_gemm(cuda, trans, M, N, K, alpha, beta, cmode, "int")
    assert np.isfinite(res).all()
    assert np.array_equal(res.astype(np.float64), ref), np.abs(res - ref).max()


# ---------------------------------------------------------------- rounding on real data
ROUNDING_SHAPES = [(False, 1, 16, 36), (False, 77, 48, 100), (False, 65, 256, 520),
                   (False, 63, 144, 1100), (True, 4, 16, 33), (True, 68, 48, 100),
                   (True, 60, 256, 520), (True, 68, 144, 1100)]


@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
@pytest.mark.parametrize("trans,M,N,K", ROUNDING_SHAPES, ids=[case_id(c) for c in ROUNDING_SHAPES])
def test_normal_data_within_dot_product_bound(trans, M, N, K, alpha, beta, cuda):
    cmode = C_MODES[(M + N // 16 + K + int(2 * alpha)) % len(C_MODES)]
    res, ref, mag = run_gemm(cuda, trans, M, N, K, alpha, beta, cmode, "normal")
    assert np.isfinite(res).all()
    ratio = float((np.abs(res - ref) / ((K + 8) * EPS * mag)).max())
    print(f"gemm_skinny {case_id((trans, M, N, K))} alpha={alpha} beta={beta}: "
          f"max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"max |err| / bound = {ratio:.4f}"


# ---------------------------------------------------------------- determinism
DETERMINISM_SHAPES = [(False, 65, 32, 100), (False, 77, 144, 1100), (True, 68, 256, 520)]


@pytest.mark.parametrize("trans,M,N,K", DETERMINISM_SHAPES,
                         ids=[case_id(c) for c in DETERMINISM_SHAPES])
def test_deterministic_and_independent_of_workspace(trans, M, N, K, cuda):
    rng = np.random.default_rng(seed_of("det", trans, M, N, K))
    A = torch.from_numpy(draw(rng, (K, M) if trans else (M, K), "normal")).to(cuda)
    B = torch.from_numpy(draw(rng, (K, N), "normal")).to(cuda)
    C0 = torch.from_numpy(draw(rng, (M, N), "normal")).to(cuda)
    check_split(M, N, K)
    outs = []
    for fill in (0xFF, 0xFF, 0x00):
        poison_workspace(cuda, fill)
        outs.append(linalg.gemm_skinny(A, B, trans, -2.0, 1.0, C=C0.clone()))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


# ---------------------------------------------------------------- layouts the wrapper takes
def test_one_row_a_as_slice(cuda):
    """A one-row A (torch reports an arbitrary row stride for it) passed as a slice."""
    rng = np.random.default_rng(5)
    big = draw(rng, (8, 36), "int")
    b = draw(rng, (36, 32), "int")
    C = linalg.gemm_skinny(torch.from_numpy(big).to(cuda)[5:6], torch.from_numpy(b).to(cuda), False)
    assert np.array_equal(C.cpu().numpy().astype(np.float64),
                          big[5:6].astype(np.float64) @ b.astype(np.float64))
    # and a fresh (1, K) tensor, a one-row B (K = 1, transposed form) and a one-row C
    a1 = draw(rng, (1, 8), "int")
    b1 = draw(rng, (1, 16), "int")
    C = linalg.gemm_skinny(torch.from_numpy(a1).to(cuda), torch.from_numpy(b1).to(cuda), True)
    assert np.array_equal(C.cpu().numpy().astype(np.float64),
                          a1.T.astype(np.float64) @ b1.astype(np.float64))


@pytest.mark.parametrize("trans", [False, True], ids=["N", "T"])
def test_column_sliced_operands_are_not_misread(trans, cuda):
    """A[:, ::2] and B[:, ::2] have a column stride of 2: the product of the view, not
    of the memory behind it."""
    rng = np.random.default_rng(6)
    M, N, K = 68, 32, 36
    aw = draw(rng, (K, 2 * M) if trans else (M, 2 * K), "int")
    bw = draw(rng, (K, 2 * N), "int")
    A, B = torch.from_numpy(aw).to(cuda)[:, ::2], torch.from_numpy(bw).to(cuda)[:, ::2]
    C = linalg.gemm_skinny(A, B, trans)
    a, b = aw[:, ::2].astype(np.float64), bw[:, ::2].astype(np.float64)
    assert np.array_equal(C.cpu().numpy().astype(np.float64), (a.T if trans else a) @ b)


def test_bad_c_is_rejected(cuda):
    A = torch.ones((8, 8), device=cuda)
    B = torch.ones((8, 32), device=cuda)
    bad = {
        "shape": torch.zeros((8, 16), device=cuda),
        "rows": torch.zeros((4, 32), device=cuda),
        "1-D": torch.zeros(8 * 32, device=cuda),
        "dtype": torch.zeros((8, 32), device=cuda, dtype=torch.float64),
        "device": torch.zeros((8, 32)),
        "column stride": torch.zeros((8, 64), device=cuda)[:, ::2],
        "transposed": torch.zeros((32, 8), device=cuda).t(),
    }
    for what, C in bad.items():
        with pytest.raises(ValueError, match="C must be"):
            linalg.gemm_skinny(A, B, False, C=C)
        assert not bool(C.any()), what
    with pytest.raises(ValueError):
        linalg.gemm_skinny(torch.ones(8, device=cuda), B, False)


# ---------------------------------------------------------------- rejections
def test_gemm_rejections(cuda):
    def ones(*shape):
        return torch.ones(shape, device=cuda)
    for A, B, trans in [(ones(8, 8), ones(8, 24), False),      # N = 24
                        (ones(8, 8), ones(8, 272), False),     # N = 272
                        (ones(8, 8), ones(12, 16), False),     # inner dimensions differ
                        (ones(8, 8), ones(12, 16), True),
                        (ones(8, 6), ones(8, 16), True),       # (T): M % 4 != 0
                        (ones(8, 6), ones(6, 16), False)]:     # (N): K % 4 != 0
        with pytest.raises(ValueError):
            linalg.gemm_skinny(A, B, trans)


def test_short_workspace_is_reported_and_c_untouched(cuda):
    M, N, K = 65, 32, 520
    L = _lib.lib()
    need = L.deig_gemm_skinny_workspace(M, N, K)
    assert need > 0
    A, B = torch.ones((M, K), device=cuda), torch.ones((K, N), device=cuda)
    out = Out(M, N, "contig", cuda, init=np.full((M, N), SENT))
    ws = linalg._workspace(cuda, need)
    for ptr, nbytes in [(ws.data_ptr(), need - 4), (ws.data_ptr(), 0), (None, 0)]:
        with torch.cuda.device(cuda):
            rc = L.deig_gemm_skinny_f32(0, A.data_ptr(), K, B.data_ptr(), N, out.view.data_ptr(),
                                        N, M, N, K, ctypes.c_float(1.0), ctypes.c_float(0.0), ptr,
                                        nbytes, linalg._stream(cuda))
        assert rc == _lib.DEIG_EWORKSPACE, _lib.last_error()
        assert _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out.flat == float(SENT)).all())


# ================================================================ projection
def project_ratio(Y, x, w):
    """max |Y - X W| over the derived bound (alpha = 1, beta = 0, K = d)."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    bound = (x.shape[1] + 8) * EPS * (np.abs(x64) @ np.abs(w64))
    err = np.abs(Y.astype(np.float64) - x64 @ w64)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), err).max())


@pytest.mark.parametrize("k", [1, 15, 16, 17, 128, 129, 255, 256])
def test_project_edges(k, cuda):
    """k on both sides of the padded-and-cropped / direct switch and above 128; n and d
    tails; d = 516 is split-K.  W row-major and column-major in turn."""
    worst = 0.0
    for i, (n, d) in enumerate((n, d) for n in (1, 65, 130) for d in (4, 36, 516)):
        rng = np.random.default_rng(seed_of("proj", n, d, k))
        x, w = draw(rng, (n, d), "normal"), draw(rng, (d, k), "normal")
        W = torch.from_numpy(w).to(cuda)
        if i % 2:
            W = W.t().contiguous().t()
        poison_workspace(cuda)
        Y = linalg.project(torch.from_numpy(x).to(cuda), W)
        assert tuple(Y.shape) == (n, k) and Y.dtype == torch.float32
        y = Y.cpu().numpy()
        assert np.isfinite(y).all(), (n, d)
        ratio = project_ratio(y, x, w)
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"n={n} d={d}: max |err| / bound = {ratio:.4f}"
    print(f"project k={k}: max |err| / bound = {worst:.4f}")


def test_project_split_k_writes_straight_into_y(cuda):
    n, d, k = 70, 1028, 32  # k % 16 == 0: no crop; 33 chunks in 4 slices
    assert _lib.lib().deig_gemm_skinny_workspace(n, k, d) == 4 * n * k * 4
    rng = np.random.default_rng(11)
    x, w = draw(rng, (n, d), "normal"), draw(rng, (d, k), "normal")
    poison_workspace(cuda)
    y = linalg.project(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)).cpu().numpy()
    ratio = project_ratio(y, x, w)
    print(f"project n={n} d={d} k={k}: max |err| / bound = {ratio:.4f}")
    assert np.isfinite(y).all() and ratio <= 1.0, ratio


def test_project_d_not_a_multiple_of_4(cuda):
    """The wrapper pads d = 37 to 40; what lies behind X's 37 columns must not enter."""
    rng = np.random.default_rng(12)
    x, w = draw(rng, (65, 37), "normal"), draw(rng, (37, 5), "normal")
    X = padded_view(x, 3, cuda)  # row stride 40, NaN in columns 37..39
    assert X.stride() == (40, 1)
    y = linalg.project(X, torch.from_numpy(w).to(cuda)).cpu().numpy()
    assert y.shape == (65, 5) and np.isfinite(y).all()
    # the zero padding adds exact zeros: the bound of d = 37 holds
    assert project_ratio(y, x, w) <= 1.0


def raw_project(dev, x, w, ymode):
    """deig_project_f32 on strided operands: ldx = d + 4 and ldw = d + 8 with NaN in the
    padding, Y inside a sentinel-filled allocation, the workspace poisoned."""
    n, d = x.shape
    k = w.shape[1]
    X = padded_view(x, 4, dev)
    Wc = padded_view(np.ascontiguousarray(w.T), 8, dev)  # (k, d + 8): column-major W
    out = Out(n, k, ymode, dev)
    L = _lib.lib()
    nbytes = L.deig_project_workspace(n, d, k)
    ws = linalg._workspace(dev, max(nbytes, POISON_BYTES))
    ws.fill_(0xFF)
    with torch.cuda.device(dev):
        rc = L.deig_project_f32(X.data_ptr(), n, d, d + 4, Wc.data_ptr(), k, d + 8,
                                out.view.data_ptr(), out.ld, ws.data_ptr(), nbytes,
                                linalg._stream(dev))
    assert rc == _lib.DEIG_OK, _lib.last_error()
    y, untouched = out.read()
    assert untouched, "wrote outside Y"
    return y


@pytest.mark.parametrize("ymode", ["pad3", "pad4"])
@pytest.mark.parametrize("d", [36, 516])
@pytest.mark.parametrize("k", [1, 16, 17, 128])
def test_project_raw_strided(k, d, ymode, cuda):
    """ldy = k + 4 takes the direct path when k % 16 == 0, ldy = k + 3 never does."""
    rng = np.random.default_rng(seed_of("raw", k, d, ymode))
    x, w = draw(rng, (65, d), "normal"), draw(rng, (d, k), "normal")
    y = raw_project(cuda, x, w, ymode)
    assert np.isfinite(y).all()
    ratio = project_ratio(y, x, w)
    assert ratio <= 1.0, f"max |err| / bound = {ratio:.4f}"


@pytest.mark.parametrize("n,d,k", [(65, 516, 17), (130, 36, 256), (70, 1028, 32)])
def test_project_integer_data_is_exact(n, d, k, cuda):
    rng = np.random.default_rng(seed_of("pint", n, d, k))
    x, w = draw(rng, (n, d), "int"), draw(rng, (d, k), "int")
    ref = x.astype(np.float64) @ w.astype(np.float64)
    poison_workspace(cuda)
    y = linalg.project(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)).cpu().numpy()
    assert np.array_equal(y.astype(np.float64), ref)
    assert np.array_equal(raw_project(cuda, x, w, "pad4").astype(np.float64), ref)
    assert np.array_equal(raw_project(cuda, x, w, "pad3").astype(np.float64), ref)


def test_project_rejections(cuda):
    X = torch.ones((10, 8), device=cuda)
    for k in (0, 257):
        with pytest.raises(ValueError):
            linalg.project(X, torch.ones((8, k), device=cuda))
    with pytest.raises(ValueError):
        linalg.project(X, torch.ones((12, 2), device=cuda))
