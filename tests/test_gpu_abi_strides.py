"""The solver-era entry points of include/deig.h - eigensolvers, sweeps, two-pass Oja,
projection, the fp32 / shifted / centred / uint8 covariances - through the C ABI with
leading dimensions other than the extent.

Every case runs on padded storage: NaN (0xFF for bytes) behind every input row, a sentinel
behind every output row and behind the last result element, a workspace of query size filled
with 0xA5 plus a canary tail.  It asserts the return code, the project's accuracy bars
against a float64 numpy reference of the same operation, finite results, bit-identical
padding, an unchanged canary, and bit equality with the same call on contiguous storage (ld =
extent, same workspace size, same stream): a leading dimension moves addresses, not the order
of the arithmetic.  The one place where the library picks another kernel by ld / alignment
and the bits may differ is named where the comparison is dropped (the eigenvalues of a
float32 S for ldv % 4 != 0 or a V off the 16-byte grid: rr.hip rq_launch).  Combinations the
library refuses (include/deig.h) must come back DEIG_EINVAL with a message and with every
output and the workspace untouched.

Bars (none new): ||P - P_ref||_F <= 1e-4, eigenvalues rtol 1e-5, max |V^T V - I| <= 1e-5
(2e-5 for k > 128, tests/test_gpu_general_solver.py), eigenvalues ascending; SYRK 2e-6 /
_split3_tol(n) (tests/test_gpu_kernels.py); sweeps 2e-6 and the per-mode bars of
test_sym_apply_* / test_sym_power_fused_chain there; Oja: check_oja's
(tests/test_gpu_single_column.py); projection: project_ratio (tests/test_gpu_skinny.py);
shifted / centred covariance: 1e-5 max|centred cov| + 1e-12 max|ref| (tests/test_gpu_f64flow.py,
tests/test_gpu_pca_kernels.py); uint8: exact (tests/test_gpu_u8.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.test_gpu_kernels import _split3_tol
from tests.test_gpu_skinny import project_ratio

pytestmark = pytest.mark.gpu

P_TOL, EV_TOL = 1e-4, 1e-5
CANARY = 1 << 16
FILL = 0xA5
SENTINEL = 777.0
NAN = float("nan")
TOL, MAX_SWEEPS = 1e-6, 300  # the Python wrappers' defaults (linalg.DEFAULT_*)


def _L():
    from distributed_eigenspaces_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Buf:
    """n rows of m elements at stride ld in a flat device buffer that starts ``off`` elements
    before the first row and runs ``tail`` elements past the last one.  ``data`` (n x m) fills
    the rows; everything else holds ``fill``."""

    def __init__(self, n, m, ld, cuda, dtype=torch.float32, fill=SENTINEL, off=0, tail=8, data=None):
        self.n, self.m, self.ld, self.off = n, m, ld, off
        self.flat = torch.full((off + n * ld + tail,), fill, dtype=dtype, device=cuda)
        if data is not None:
            if isinstance(data, np.ndarray):
                data = torch.from_numpy(np.ascontiguousarray(data))
            self.rows()[:] = data.to(device=cuda, dtype=dtype)
        self.before = self.flat.clone()
        self.ptr = self.flat.data_ptr() + off * self.flat.element_size()

    def rows(self):
        return self.flat[self.off:self.off + self.n * self.ld].view(self.n, self.ld)[:, :self.m]

    def numpy(self):
        return self.rows().cpu().numpy()

    def padding_intact(self):
        """Every element outside the n x m result holds the bits it held before the call."""
        mask = torch.ones(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        mask[self.off:self.off + self.n * self.ld].view(self.n, self.ld)[:, :self.m] = False
        return torch.equal(_bits(self.flat)[mask], _bits(self.before)[mask])

    def untouched(self):
        return torch.equal(_bits(self.flat), _bits(self.before))

    def same_result(self, other):
        return torch.equal(_bits(self.rows()), _bits(other.rows()))


class Ws:
    def __init__(self, nbytes, cuda):
        self.nbytes = int(nbytes)
        self.t = torch.full((max(self.nbytes, 1) + CANARY,), FILL, dtype=torch.uint8, device=cuda)
        self.ptr = self.t.data_ptr()

    def canary_intact(self):
        return bool((self.t[self.nbytes:] == FILL).all())

    def untouched(self):
        return bool((self.t == FILL).all())


def _inputs(a, ld, cuda, off=0):
    """A read-only operand: NaN (0xFF for bytes) in the padding, which must stay as it is."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    fill = 255 if t.dtype == torch.uint8 else NAN
    return Buf(t.shape[0], t.shape[1], ld, cuda, dtype=t.dtype, fill=fill, off=off, tail=8, data=t)


# ================================================================ eigensolvers
def _spectrum_matrix(d, k, seed, top=None):
    """U diag(lam) U^T with the spectrum of test_gpu_kernels.test_topk_random_spectra; ``top``
    replaces the largest eigenvalue (the dominant pair of the deflation cases)."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.concatenate([np.linspace(10, 5, k), np.linspace(1, 0.01, d - k)])
    if top is not None:
        lam[0] = top
    S = (U * lam) @ U.T
    return ((S + S.T) / 2).astype(np.float32)


class Solve:
    """One deig_topk_sym_* / deig_projavg_topk_* call on padded storage."""

    def __init__(self, cuda, d, k, *, ldv, v_off=0, S=None, lds=None, s_off=0, stype=None, Wt=None,
                 ldw=None, scale=1.0, q0=None, ldq0=0, opts=None, entry="ex"):
        L = _L()
        lib = L.lib()
        self.d, self.k = d, k
        self.V = Buf(k, d, ldv, cuda, off=v_off)           # column-major d x k
        self.ev = Buf(1, k, k, cuda)
        self.q0 = None if q0 is None else _inputs(q0.T, ldq0, cuda)
        k0 = 0 if q0 is None else q0.shape[1]
        qp = None if q0 is None else self.q0.ptr
        o = opts if opts is not None else L.solver_opts()
        sweeps, resid = ctypes.c_int(-1), ctypes.c_float(-1.0)
        if S is not None:
            stype = L.DEIG_F64 if S.dtype == np.float64 else L.DEIG_F32
            self.S = _inputs(S, lds, cuda, off=s_off)
            self.ws = Ws(lib.deig_topk_workspace_ex(d, k, 0, stype, ctypes.byref(o)), cuda)
            if entry == "f32":
                assert stype == L.DEIG_F32 and opts is None
                assert self.ws.nbytes == lib.deig_topk_workspace(d, k, 0)
                self.rc = lib.deig_topk_sym_f32(self.S.ptr, d, lds, k, 0, MAX_SWEEPS, TOL, qp, k0, ldq0,
                                                self.V.ptr, ldv, self.ev.ptr, ctypes.byref(sweeps),
                                                ctypes.byref(resid), self.ws.ptr, self.ws.nbytes, _stream())
            else:
                self.rc = lib.deig_topk_sym_ex(self.S.ptr, stype, d, lds, k, 0, MAX_SWEEPS, TOL, qp, k0,
                                               ldq0, self.V.ptr, ldv, self.ev.ptr, ctypes.byref(sweeps),
                                               ctypes.byref(resid), ctypes.byref(o), self.ws.ptr,
                                               self.ws.nbytes, _stream())
        else:
            self.S = _inputs(Wt, ldw, cuda)
            mk = Wt.shape[0]
            self.ws = Ws(lib.deig_projavg_workspace_ex(d, mk, k, 0, ctypes.byref(o)), cuda)
            if entry == "f32":
                assert self.ws.nbytes == lib.deig_projavg_workspace(d, mk, k, 0)
                self.rc = lib.deig_projavg_topk_f32(self.S.ptr, d, mk, ldw, scale, k, 0, MAX_SWEEPS, TOL,
                                                    qp, k0, ldq0, self.V.ptr, ldv, self.ev.ptr,
                                                    ctypes.byref(sweeps), ctypes.byref(resid),
                                                    self.ws.ptr, self.ws.nbytes, _stream())
            else:
                self.rc = lib.deig_projavg_topk_ex(self.S.ptr, d, mk, ldw, scale, k, 0, MAX_SWEEPS, TOL,
                                                   qp, k0, ldq0, self.V.ptr, ldv, self.ev.ptr,
                                                   ctypes.byref(sweeps), ctypes.byref(resid),
                                                   ctypes.byref(o), self.ws.ptr, self.ws.nbytes, _stream())
        self.err = L.last_error()
        torch.cuda.synchronize()
        self.sweeps = sweeps.value

    def check(self, w, Vr, what, ev_atol=0.0):
        """The bars against the float64 eigenpairs (w ascending, Vr), and the storage."""
        assert self.rc == 0, f"{what}: rc {self.rc}: {self.err}"
        V = self.V.numpy().T.astype(np.float64)
        ev = self.ev.numpy()[0].astype(np.float64)
        assert np.isfinite(V).all() and np.isfinite(ev).all(), f"{what}: NaN leaked in"
        dist = ref_cpu.projector_distance(V, Vr)
        orth = np.abs(V.T @ V - np.eye(self.k)).max()
        everr = np.max(np.abs(ev - w) / np.abs(w))
        print(f"{what}: {self.sweeps} sweeps, ||P-P_ref||_F {dist:.3e}, max|V^T V - I| {orth:.3e}, "
              f"eigenvalue rel err {everr:.3e}")
        assert dist <= P_TOL, f"{what}: ||P - P_ref||_F = {dist:.3e}"
        np.testing.assert_allclose(ev, w, rtol=EV_TOL, atol=ev_atol, err_msg=what)
        assert np.all(np.diff(ev) >= -1e-6 * np.abs(ev).max()), f"{what}: eigenvalues not ascending"
        assert orth <= (2e-5 if self.k > 128 else 1e-5), f"{what}: max |V^T V - I| = {orth:.3e}"
        self.check_storage(what)

    def check_storage(self, what):
        assert self.V.padding_intact(), f"{what}: wrote outside V's columns"
        assert self.ev.padding_intact(), f"{what}: wrote behind evals[k-1]"
        assert self.S.untouched(), f"{what}: the operator was written"
        assert self.q0 is None or self.q0.untouched(), f"{what}: the warm start was written"
        assert self.ws.canary_intact(), f"{what}: wrote past the workspace"

    def check_rejected(self, what, *words):
        L = _L()
        assert self.rc == L.DEIG_EINVAL, f"{what}: rc {self.rc}: {self.err}"
        assert self.err, f"{what}: no message"
        for w in words:
            assert w in self.err, (what, w, self.err)
        assert self.V.untouched() and self.ev.untouched(), f"{what}: outputs written by a rejected call"
        assert self.ws.untouched(), f"{what}: GPU work before the rejection"


def _ref(S32, k):
    return ref_cpu.top_k_eigh(S32.astype(np.float64), k)


@pytest.mark.parametrize("case", ["f32_entry", "ex_f32", "ex_f64"])
def test_topk_in_place_padded_by_4(case, cuda):
    """lds = ldv = d + 4, warm start with ldq0 = d + 12: every vector path keeps its
    alignment, so every output - the eigenvalues too - has the contiguous call's bits."""
    d, k, k0 = 256, 16, 8
    S = _spectrum_matrix(d, k, seed=d + k)
    if case == "ex_f64":
        S = S.astype(np.float64)
    q0 = np.random.default_rng(3).standard_normal((d, k0)).astype(np.float32)
    entry = "f32" if case == "f32_entry" else "ex"
    pad = Solve(cuda, d, k, S=S, lds=d + 4, ldv=d + 4, q0=q0, ldq0=d + 12, entry=entry)
    pad.check(*_ref(S, k), f"topk {case} padded by 4")
    flat = Solve(cuda, d, k, S=S, lds=d, ldv=d, q0=q0, ldq0=d, entry=entry)
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    assert pad.ev.same_result(flat.ev), "eigenvalues differ from the contiguous call"


@pytest.mark.parametrize("ldv_pad,v_off", [(1, 0), (3, 0), (4, 1)])
def test_topk_in_place_odd_ldv(ldv_pad, v_off, cuda):
    """ldv = d + 1, d + 3, and a V one float off the 16-byte grid: V keeps the contiguous
    call's bits; the eigenvalues come from the plain Rayleigh-quotient kernels."""
    d, k, k0 = 256, 16, 8
    S = _spectrum_matrix(d, k, seed=d + k)
    q0 = np.random.default_rng(3).standard_normal((d, k0)).astype(np.float32)
    pad = Solve(cuda, d, k, S=S, lds=d + 4, ldv=d + ldv_pad, v_off=v_off, q0=q0, ldq0=d + 12)
    pad.check(*_ref(S, k), f"topk ldv=d+{ldv_pad} V offset {v_off}")
    flat = Solve(cuda, d, k, S=S, lds=d, ldv=d, q0=q0, ldq0=d)
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    # no bit comparison of the eigenvalues: rr.hip rq_launch (`const bool mfma = ... ldv % 4
    # == 0 ... aligned16(V)`) takes rq_part_kernel here and rq_mfma_kernel for the contiguous
    # call - double sums in another order; the float64 bar above holds for both


@pytest.mark.parametrize("ldv_pad", [4, 1])
@pytest.mark.parametrize("algo", ["auto", "fp32"])
def test_topk_deflation(algo, ldv_pad, cuda):
    """One eigenvalue 1000 x the largest of the rest (theta_1 >= 64 theta_k): the dominant
    pair is locked and the others iterated on the deflated operator, formed in double -
    folded into the sweep image (auto) or into the fp32 sweep's copy of S (DEIG_SWEEP_FP32).
    Both read the locked column of V by element: any ldv."""
    L = _L()
    d, k = 256, 8
    S = _spectrum_matrix(d, k, seed=d + k, top=1e4)
    w, Vr = _ref(S, k)
    assert w[-1] >= 64 * w[0]
    code = {"auto": L.DEIG_SWEEP_AUTO, "fp32": L.DEIG_SWEEP_FP32}[algo]
    pad = Solve(cuda, d, k, S=S, lds=d + 4, ldv=d + ldv_pad, opts=L.solver_opts(sweep_algo=code))
    what = f"deflation {algo} ldv=d+{ldv_pad}"
    pad.check(w, Vr, what)
    flat = Solve(cuda, d, k, S=S, lds=d, ldv=d, opts=L.solver_opts(sweep_algo=code))
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    if ldv_pad % 4 == 0:  # else rr.hip rq_launch's `mfma` branch, as in test_topk_in_place_odd_ldv
        assert pad.ev.same_result(flat.ev), "eigenvalues differ from the contiguous call"


@pytest.mark.parametrize("ldv_pad", [8, 1])
@pytest.mark.parametrize("algo", ["auto", "fp32"])
def test_topk_block_locking_explicit(algo, ldv_pad, cuda):
    """k = 160 > 128 on an explicit S: two blocks, the first one's pairs locked in V and
    deflated through the sweep image (auto) or the fp32 sweep's copy of S - any ldv.
    (k > 128 never takes rq_launch's MFMA form, so the eigenvalues keep their bits for an
    odd ldv as well.)"""
    L = _L()
    code = {"auto": L.DEIG_SWEEP_AUTO, "fp32": L.DEIG_SWEEP_FP32}[algo]
    d, k = 512, 160
    rng = np.random.default_rng(d + k)
    U, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.concatenate([np.linspace(10.0, 5.0, k), np.linspace(2.0, 0.0, d - k)])  # general_solver's
    S = (U * lam) @ U.T
    S = ((S + S.T) / 2).astype(np.float32)
    pad = Solve(cuda, d, k, S=S, lds=d + 4, ldv=d + ldv_pad, opts=L.solver_opts(sweep_algo=code))
    pad.check(*_ref(S, k), f"block locking {algo} ldv=d+{ldv_pad}")
    flat = Solve(cuda, d, k, S=S, lds=d, ldv=d, opts=L.solver_opts(sweep_algo=code))
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    assert pad.ev.same_result(flat.ev), "eigenvalues differ from the contiguous call"


def _projavg_case(d, k, seed):
    """What the server sees: two workers' estimates of one k-dimensional eigenspace, each
    the orthonormalised sum of the true basis and its own noise (column norm 0.5).  The
    average of the two projectors has eigenvalues (1 + cos theta_i) / 2 on top and
    (1 - cos theta_i) / 2 below, theta_i the principal angles between the estimates: k
    distinct eigenvalues near 1 and a clear gap at k (asserted).  Returns Wt (2k x d,
    float32), the bases and the float64 reference of the rounded bases."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((d, k)))[0]
    bases = [np.linalg.qr(U + 0.5 / np.sqrt(d) * rng.standard_normal((d, k)))[0].astype(np.float32)
             for _ in range(2)]
    w_all = np.linalg.eigvalsh(ref_cpu.projector_average([b.astype(np.float64) for b in bases], 2))
    assert w_all[-k] - w_all[-k - 1] >= 0.25, "no gap at k"
    w, V = ref_cpu.server_topk([b.astype(np.float64) for b in bases], k, 2)
    return np.vstack([b.T for b in bases]), bases, w, V


@pytest.mark.parametrize("ldv_pad", [8, 1])
def test_projavg_block_locking(ldv_pad, cuda):
    """The projector average of m = 2 bases with k = 160 > 128 (ldw = d + 4, NaN padding): the
    locked block is deflated by products with V itself, which therefore has to be 16-byte
    aligned with ldv % 4 == 0 - ldv = d + 1 is refused before any GPU work."""
    d, k = 512, 160
    Wt, _, w, Vr = _projavg_case(d, k, seed=11)
    pad = Solve(cuda, d, k, Wt=Wt, ldw=d + 4, scale=0.5, ldv=d + ldv_pad)
    what = f"projavg k=160 ldv=d+{ldv_pad}"
    if ldv_pad % 4:
        pad.check_rejected(what, "projavg", "k > 128", "ldv % 4 == 0")
        return
    pad.check(w, Vr, what, ev_atol=1e-6)  # atol: test_projector_average_k_above_128's
    flat = Solve(cuda, d, k, Wt=Wt, ldw=d, scale=0.5, ldv=d)
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    assert pad.ev.same_result(flat.ev), "eigenvalues differ from the contiguous call"


@pytest.mark.parametrize("entry", ["f32", "ex"])
def test_projavg_single_block_any_ldv(entry, cuda):
    """k <= 128 on the implicit operator: nothing is locked, V is only written - an odd ldv, a
    warm start with ldq0 = d + 12."""
    d, k = 256, 16
    Wt, bases, w, Vr = _projavg_case(d, k, seed=5)
    q0 = bases[0][:, :8].copy()
    pad = Solve(cuda, d, k, Wt=Wt, ldw=d + 4, scale=0.5, ldv=d + 1, q0=q0, ldq0=d + 12, entry=entry)
    pad.check(w, Vr, f"projavg {entry} k=16 ldv=d+1", ev_atol=1e-6)
    flat = Solve(cuda, d, k, Wt=Wt, ldw=d, scale=0.5, ldv=d, q0=q0, ldq0=d, entry=entry)
    assert flat.rc == 0
    assert pad.V.same_result(flat.V) and pad.ev.same_result(flat.ev)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("d,k,k0", [(102, 5, 3), (17, 3, 2)])
def test_topk_staged_element_alignment(d, k, k0, f64, cuda):
    """d % 4 != 0: S is staged, so any lds >= d and element alignment are promised - S one
    element into its buffer, lds = d + 3, ldv = d + 1, ldq0 = d + 5.  V and the eigenvalues
    are computed in the workspace: the contiguous call's bits, both."""
    S = _spectrum_matrix(d, k, seed=d + k)
    if f64:
        S = S.astype(np.float64)
    q0 = np.random.default_rng(d).standard_normal((d, k0)).astype(np.float32)
    pad = Solve(cuda, d, k, S=S, lds=d + 3, s_off=1, ldv=d + 1, q0=q0, ldq0=d + 5)
    pad.check(*_ref(S, k), f"staged d={d} f64={f64}")
    flat = Solve(cuda, d, k, S=S, lds=d, ldv=d, q0=q0, ldq0=d)
    assert flat.rc == 0
    assert pad.V.same_result(flat.V), "V differs from the contiguous call"
    assert pad.ev.same_result(flat.ev), "eigenvalues differ from the contiguous call"


def test_topk_batch_padded(cuda):
    """W = 3 problems, lds = d + 4, ldv = d + 8: status 0 each, the bars each, and each
    problem's bits those of its own single padded solve."""
    L = _L()
    lib = L.lib()
    W, d, k, lds, ldv = 3, 256, 16, 260, 264
    Ss = [_spectrum_matrix(d, k, seed=100 + i) for i in range(W)]
    Sb = [_inputs(S, lds, cuda) for S in Ss]
    Vb = [Buf(k, d, ldv, cuda) for _ in range(W)]
    Eb = [Buf(1, k, k, cuda) for _ in range(W)]
    o = L.solver_opts()
    ws = Ws(lib.deig_topk_batch_workspace(W, d, k, 0, L.DEIG_F32, ctypes.byref(o)), cuda)
    arr = lambda bs: (ctypes.c_void_p * W)(*[b.ptr for b in bs])  # noqa: E731
    sweeps, resid, status = (ctypes.c_int * W)(), (ctypes.c_float * W)(), (ctypes.c_int * W)(9, 9, 9)
    rc = lib.deig_topk_sym_batch_ex(W, arr(Sb), L.DEIG_F32, d, lds, k, 0, MAX_SWEEPS, TOL, arr(Vb), ldv,
                                    arr(Eb), sweeps, resid, status, ctypes.byref(o), ws.ptr, ws.nbytes,
                                    _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    assert list(status) == [0] * W
    assert ws.canary_intact()
    for i in range(W):
        one = Solve(cuda, d, k, S=Ss[i], lds=lds, ldv=ldv)
        one.check(*_ref(Ss[i], k), f"single padded solve {i}")
        assert Vb[i].padding_intact() and Eb[i].padding_intact() and Sb[i].untouched()
        assert Vb[i].same_result(one.V), f"problem {i}: V differs from its single solve"
        assert Eb[i].same_result(one.ev), f"problem {i}: eigenvalues differ from its single solve"
        assert sweeps[i] == one.sweeps


# ================================================================ sweeps
SWEEP_SHAPES = [(60, 16), (520, 80), (2048, 64)]  # split-K slices: 1, 2, 8
SWEEP_MODES = ["exact", "round_q", "fast", "half"]


def _sweep_cases():
    for d, p in SWEEP_SHAPES:
        for mode in SWEEP_MODES:
            if mode == "half" and p != 64:
                continue
            for lq, ly in ((4, 4), (1, 3)):
                yield pytest.param(d, p, mode, "bf16x6", lq, ly, id=f"{d}-{p}-{mode}-ldq+{lq}-ldy+{ly}")
        yield pytest.param(d, p, "exact", "fp32", 4, 4, id=f"{d}-{p}-fp32")


def _sweep_code(mode, algo):
    L = _L()
    if algo == "fp32":
        return L.DEIG_SWEEP_FP32
    return L.DEIG_SWEEP_BF16X6 | {"exact": 0, "round_q": L.DEIG_SWEEP_ROUND_Q, "fast": L.DEIG_SWEEP_FAST,
                                  "half": L.DEIG_SWEEP_HALF}[mode]


def _two_pieces(x):
    """h + m: the two leading bf16 pieces of a float32 array (round to nearest even)."""
    t = torch.from_numpy(x)
    h = t.to(torch.bfloat16).float()
    return (h + (t - h).to(torch.bfloat16).float()).numpy()


def _sweep_inputs(d, p, seed, scaled=False):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d))
    S = ((A + A.T) * (0.5 / np.sqrt(d) if scaled else 0.5)).astype(np.float32)
    return S, rng.standard_normal((d, p)).astype(np.float32)


def _check_sweep_mode(Y, Qr, S, Q, mode, alpha, what):
    """test_gpu_kernels' bars of one sweep in ``mode``: Y against float64 products of the
    operands the mode takes, Q' against the two-piece rounding."""
    S64 = S.astype(np.float64)
    if mode == "exact":
        assert np.array_equal(Qr, Q), f"{what}: Q was written"
    else:
        assert np.all(np.abs(Qr - Q) <= 2.0 ** -17 * np.abs(Q) * 1.0001), f"{what}: rounding exceeds 2^-17"
        assert np.array_equal(_two_pieces(Qr), Qr), f"{what}: Q' is not two bf16 pieces"
    ref = alpha * (S64 @ Qr.astype(np.float64))
    scale = np.abs(ref).max()
    err = np.abs(Y - ref).max() / scale
    if mode in ("exact", "round_q"):
        assert err <= 2e-6, f"{what}: rel err {err:.3e}"
    elif mode == "fast":
        ref2 = alpha * (_two_pieces(S).astype(np.float64) @ Qr.astype(np.float64))
        assert np.abs(Y - ref2).max() / scale <= 1e-5, f"{what}: vs S'Q'"
        assert err <= 6e-5, f"{what}: vs SQ'"
    else:
        Sh = torch.from_numpy(S).to(torch.bfloat16).double().numpy()
        Qh = torch.from_numpy(Q).to(torch.bfloat16).double().numpy()
        assert np.abs(Y - alpha * (Sh @ Qh)).max() / scale <= 1e-5, f"{what}: vs h(S)h(Q)"
        assert err <= 1e-2, f"{what}: vs SQ'"
    print(f"{what}: rel err {err:.3e}")


class Sweep:
    def __init__(self, cuda, S, Q, lds, ldq, ldy, code, alpha=1.0, cs=None, steps=0):
        L = _L()
        lib = L.lib()
        d, p = Q.shape
        self.S = _inputs(S, lds, cuda)
        self.Q = _inputs(Q, ldq, cuda)  # ROUND_Q / FAST / HALF and the power chain write it in place
        self.Y = Buf(d, p, ldy, cuda)
        self.ws = Ws(lib.deig_sym_apply_workspace(d, p, code), cuda)
        if steps:
            self.cs = torch.from_numpy(cs).to(cuda)
            self.rc = lib.deig_sym_power_f32(self.S.ptr, d, lds, self.Q.ptr, p, ldq, self.Y.ptr, ldy,
                                             self.cs.data_ptr(), steps, code, self.ws.ptr, self.ws.nbytes,
                                             _stream())
        else:
            self.rc = lib.deig_sym_apply_f32(self.S.ptr, d, lds, self.Q.ptr, p, ldq, self.Y.ptr, ldy, alpha,
                                             code, self.ws.ptr, self.ws.nbytes, _stream())
        self.err = L.last_error()
        torch.cuda.synchronize()

    def check_storage(self, what):
        assert self.rc == 0, f"{what}: rc {self.rc}: {self.err}"
        assert self.Y.padding_intact(), f"{what}: wrote outside Y's columns"
        assert self.Q.padding_intact(), f"{what}: Q's padding changed"
        assert self.S.untouched(), f"{what}: S was written"
        assert self.ws.canary_intact(), f"{what}: wrote past the workspace"
        assert np.isfinite(self.Y.numpy()).all() and np.isfinite(self.Q.numpy()).all(), f"{what}: NaN leaked in"


@pytest.mark.parametrize("d,p,mode,algo,lq,ly", _sweep_cases())
def test_sym_apply_padded(d, p, mode, algo, lq, ly, cuda):
    S, Q = _sweep_inputs(d, p, seed=31 * d + p)
    code = _sweep_code(mode, algo)
    what = f"sym_apply[{algo} {mode}] d={d} p={p} ldq=p+{lq} ldy=p+{ly}"
    pad = Sweep(cuda, S, Q, d + 4, p + lq, p + ly, code, alpha=0.5)
    pad.check_storage(what)
    _check_sweep_mode(pad.Y.numpy().astype(np.float64), pad.Q.numpy(), S, Q, mode, 0.5, what)
    flat = Sweep(cuda, S, Q, d, p, p, code, alpha=0.5)
    assert flat.rc == 0
    assert pad.Y.same_result(flat.Y), f"{what}: Y differs from the contiguous call"
    assert pad.Q.same_result(flat.Q), f"{what}: Q' differs from the contiguous call"


def _power_cases():
    for d, p in SWEEP_SHAPES:
        for mode in SWEEP_MODES:
            if mode == "half" and p != 64:
                continue
            yield pytest.param(d, p, mode, id=f"{d}-{p}-{mode}")


@pytest.mark.parametrize("d,p,mode", _power_cases())
def test_sym_power_padded(d, p, mode, cuda):
    """Three steps of the fused chain with ldq = ldy = p + 4 and one column kept (cs <= 0),
    at test_sym_power_fused_chain's bars."""
    S, Q = _sweep_inputs(d, p, seed=d + p, scaled=True)
    cs = np.full(p, 0.5, dtype=np.float32)
    cs[3] = -1.0  # kept column
    steps = 3
    code = _sweep_code(mode, "bf16x6")
    what = f"sym_power[{mode}] d={d} p={p}"
    pad = Sweep(cuda, S, Q, d + 4, p + 4, p + 4, code, cs=cs, steps=steps)
    pad.check_storage(what)
    Qr, S64 = Q.astype(np.float64), S.astype(np.float64)
    for _ in range(steps):
        Yr = S64 @ Qr
        Qn = Yr * cs
        Qn[:, cs <= 0] = Qr[:, cs <= 0]
        Qr = Qn
    tol = {"exact": 6e-6, "round_q": 5e-5, "fast": 2e-4, "half": 2e-2}[mode]
    for name, got, ref in (("Y", pad.Y.numpy(), Yr), ("Q", pad.Q.numpy(), Qr)):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{what}: {name} rel err {err:.3e}")
        assert err <= tol, f"{what}: {name} rel err {err:.3e} > {tol:.1e}"
    if mode != "exact":
        assert np.array_equal(_two_pieces(pad.Q.numpy()), pad.Q.numpy())
    flat = Sweep(cuda, S, Q, d, p, p, code, cs=cs, steps=steps)
    assert flat.rc == 0
    assert pad.Y.same_result(flat.Y) and pad.Q.same_result(flat.Q), f"{what}: differs from the contiguous call"


# ================================================================ Oja, two-pass
def _oja_data(d, b, k, nb, seed):
    """A spiked model: k directions with standard deviations 3 .. 1.5 over noise 0.5."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((d, k)))[0]
    X = (rng.standard_normal((nb * b, k)) * np.linspace(3.0, 1.5, k)) @ U.T
    X = (X + 0.5 * rng.standard_normal((nb * b, d))).astype(np.float32)
    V0 = np.linalg.qr(rng.standard_normal((d, k)))[0].astype(np.float32)
    return X, V0


@functools.lru_cache(maxsize=None)
def _oja_ref(d, b, k, nb, eta):
    """The inputs and the float64 epoch of one shape, computed once and shared by its cases."""
    X, V0 = _oja_data(d, b, k, nb, seed=d + b + k)
    return X, V0, ref_cpu.oja_epoch(X.astype(np.float64), V0.astype(np.float64), eta, b)


OJA_ETA = 0.1


def _oja_run(cuda, X, V0, b, nb, ldx, ldv, how, orth_every):
    L = _L()
    lib = L.lib()
    d, k = V0.shape
    Xb = _inputs(X, ldx, cuda)
    Vb = Buf(k, d, ldv, cuda, data=V0.T)
    ws = Ws(lib.deig_oja_workspace(b, d, k), cuda)
    if how == "step":
        for i in range(nb):
            rc = lib.deig_oja_step_f32(Xb.ptr + 4 * i * b * ldx, b, d, ldx, OJA_ETA, Vb.ptr, k, ldv, ws.ptr,
                                       ws.nbytes, _stream())
            assert rc == 0, L.last_error()
    else:
        rc = lib.deig_oja_steps_ex(Xb.ptr, nb, b, d, ldx, OJA_ETA, Vb.ptr, k, ldv, orth_every,
                                   L.DEIG_OJA_TWO_PASS, ws.ptr, ws.nbytes, _stream())
        assert rc == 0, L.last_error()
    assert lib.deig_oja_error(ws.ptr, ws.nbytes, b, d, k, _stream()) == 0
    torch.cuda.synchronize()
    return Xb, Vb, ws


@pytest.mark.parametrize("how,orth_every", [("step", 1), ("steps", 1), ("steps", 3)])
@pytest.mark.parametrize("d,b,k", [(96, 260, 5), (260, 1040, 33)])
def test_oja_two_pass_padded(d, b, k, how, orth_every, cuda):
    """ldx = d + 4 with NaN behind every sample row, ldv = d + 3 with a sentinel behind every
    basis column; check_oja's bar against the float64 epoch."""
    nb = 3
    X, V0, Vr = _oja_ref(d, b, k, nb, OJA_ETA)
    Xb, Vb, ws = _oja_run(cuda, X, V0, b, nb, d + 4, d + 3, how, orth_every)
    what = f"oja {how} orth_every={orth_every} d={d} b={b} k={k}"
    Vg = Vb.numpy().T.astype(np.float64)
    assert np.isfinite(Vg).all(), f"{what}: NaN leaked in"
    np.testing.assert_allclose(Vg.T @ Vg, np.eye(k), atol=1e-5, err_msg=what)
    dist = ref_cpu.projector_distance(Vg, Vr)
    print(f"{what}: ||P-P_ref||_F {dist:.3e}")
    assert dist <= P_TOL, f"{what}: ||P - P_ref||_F = {dist:.3e}"
    assert Vb.padding_intact(), f"{what}: wrote outside V's columns"
    assert Xb.untouched() and ws.canary_intact()
    _, Vf, _ = _oja_run(cuda, X, V0, b, nb, d, d, how, orth_every)
    assert Vb.same_result(Vf), f"{what}: V differs from the contiguous call"


# ================================================================ projection
@pytest.mark.parametrize("k", [1, 17, 256])
@pytest.mark.parametrize("d", [64, 260])
def test_project_padded(d, k, cuda):
    """ldx = d + 4, ldw = d + 1, ldy = k + 1 for every row-tile tail n."""
    L = _L()
    lib = L.lib()
    for n in (1, 63, 65, 777):
        rng = np.random.default_rng(1000 * n + 10 * d + k)
        X = rng.standard_normal((n, d)).astype(np.float32)
        W = (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
        out = []
        for ldx, ldw, ldy in ((d + 4, d + 1, k + 1), (d, d, k)):
            Xb, Wb = _inputs(X, ldx, cuda), _inputs(W.T, ldw, cuda)
            Yb = Buf(n, k, ldy, cuda)
            ws = Ws(lib.deig_project_workspace(n, d, k), cuda)
            rc = lib.deig_project_f32(Xb.ptr, n, d, ldx, Wb.ptr, k, ldw, Yb.ptr, ldy, ws.ptr, ws.nbytes,
                                      _stream())
            torch.cuda.synchronize()
            assert rc == 0, L.last_error()
            out.append((Xb, Wb, Yb, ws))
        Xb, Wb, Yb, ws = out[0]
        what = f"project n={n} d={d} k={k}"
        Y = Yb.numpy()
        assert np.isfinite(Y).all(), f"{what}: NaN leaked in"
        ratio = project_ratio(Y, X, W)
        assert ratio <= 1.0, f"{what}: err / bound = {ratio:.3f}"
        assert Yb.padding_intact(), f"{what}: wrote outside Y's columns"
        assert Xb.untouched() and Wb.untouched() and ws.canary_intact()
        assert Yb.same_result(out[1][2]), f"{what}: Y differs from the contiguous call"


# ================================================================ covariances
SYRK_SHAPES = [(33, 64), (257, 260), (1100, 520), (64, 2052)]


def _syrk_run(cuda, X, S0, ldx, lds, code, alpha, ws_bytes=None):
    L = _L()
    lib = L.lib()
    n, d = X.shape
    Xb = _inputs(X, ldx, cuda)
    Sb = Buf(d, d, lds, cuda, data=S0)  # S0: the incoming S of DEIG_SYRK_ACCUMULATE
    ws = Ws(lib.deig_syrk_workspace_ex(n, d, code) if ws_bytes is None else ws_bytes, cuda)
    rc = lib.deig_syrk_f32_ex(Xb.ptr, n, d, ldx, alpha, Sb.ptr, lds, code, ws.ptr, ws.nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    return Xb, Sb, ws


def _syrk_case(cuda, n, d, algo, ws_rows=None):
    L = _L()
    rng = np.random.default_rng(n * 7919 + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    acc = algo == "split3_acc"
    code = {"fp32": L.DEIG_SYRK_FP32, "split3": L.DEIG_SYRK_SPLIT3,
            "split3_acc": L.DEIG_SYRK_SPLIT3 | L.DEIG_SYRK_ACCUMULATE}[algo]
    S0 = None
    if acc:  # bit-symmetric (a + b is commutative), so whichever triangle is read gives it
        A = rng.standard_normal((d, d)).astype(np.float32)
        S0 = A + A.T
    ws_bytes = None
    if ws_rows is not None:
        ws_bytes = L.lib().deig_syrk_workspace_ex(ws_rows, d, code)
        assert ws_bytes < L.lib().deig_syrk_workspace_ex(n, d, code), "one chunk would hold all rows"
    alpha = 1.0 / n
    Xb, Sb, ws = _syrk_run(cuda, X, S0, d + 4, d + 4, code, alpha, ws_bytes)
    what = f"syrk[{algo}] n={n} d={d}" + (f" chunks of {ws_rows}" if ws_rows else "")
    S = Sb.numpy().astype(np.float64)
    assert np.isfinite(S).all(), f"{what}: NaN leaked in"
    ref = ref_cpu.sigma_hat(X.astype(np.float64)) + (S0.astype(np.float64) if acc else 0.0)
    err = np.abs(S - ref).max() / np.abs(ref).max()
    tol = 2e-6 if algo == "fp32" else _split3_tol(n)
    print(f"{what}: rel err {err:.3e} (bar {tol:.0e})")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.0e}"
    assert np.array_equal(S, S.T), f"{what}: S is not bit-exactly symmetric"
    assert Sb.padding_intact(), f"{what}: wrote outside S's columns"
    assert Xb.untouched() and ws.canary_intact()
    _, Sf, _ = _syrk_run(cuda, X, S0, d, d, code, alpha, ws_bytes)
    assert Sb.same_result(Sf), f"{what}: S differs from the contiguous call"


@pytest.mark.parametrize("algo", ["fp32", "split3", "split3_acc"])
@pytest.mark.parametrize("n,d", SYRK_SHAPES)
def test_syrk_padded(n, d, algo, cuda):
    _syrk_case(cuda, n, d, algo)


@pytest.mark.parametrize("algo", ["split3", "split3_acc"])
def test_syrk_padded_two_row_chunks(algo, cuda):
    """d > 2048 (the split pass) with a workspace sized for 32 of the 64 rows, as
    tests/test_gpu_syrk_chunks.py sizes it: two chunks, the second accumulating into the
    padded S."""
    _syrk_case(cuda, 64, 2052, algo, ws_rows=32)


def _float_samples(n, d, xtype_name, seed):
    """100 + 20 N(0, 1) in the element type; returns (torch tensor, its float64 values)."""
    rng = np.random.default_rng(seed)
    x = 100.0 + 20.0 * rng.standard_normal((n + 50, d))
    t = torch.from_numpy(x).to({"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}[xtype_name])
    x64 = t.double().numpy()
    return t[:n].contiguous(), x64[:n], x64.mean(axis=0)  # the mean of the larger set: 'pooled'


def _cov_outputs(cuda, d, lds64, lds, want):
    S64 = Buf(d, d, lds64, cuda, dtype=torch.float64) if "S64" in want else None
    S32 = Buf(d, d, lds, cuda) if "S" in want else None
    return S64, S32


@pytest.mark.parametrize("xt", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("entry", ["shift", "centered"])
@pytest.mark.parametrize("n,d", [(100, 37), (1100, 260)])
def test_shifted_and_centred_covariance_padded(n, d, entry, xt, cuda):
    """ldx = d + 1 (NaN behind every row), lds64 = d + 1, lds = d + 3: both outputs at once
    and each alone; the centred form about a pooled centre, with mean_out."""
    L = _L()
    lib = L.lib()
    xtype = {"f32": L.DEIG_F32, "f64": L.DEIG_F64, "bf16": L.DEIG_BF16}[xt]
    X, x64, pooled = _float_samples(n, d, xt, seed=7 * n + d)
    own = x64.mean(axis=0)
    c = pooled if entry == "centered" else np.zeros(d)
    t = x64 - c
    ref = t.T @ t / n
    tc = x64 - own
    bar = 1e-5 * np.abs(tc.T @ tc / n).max() + 1e-12 * np.abs(ref).max()
    center = torch.from_numpy(pooled).to(cuda)
    what = f"syrk_{entry}[{xt}] n={n} d={d}"

    def run(ldx, lds64, lds, want):
        Xb = _inputs(X, ldx, cuda)
        S64, S32 = _cov_outputs(cuda, d, lds64, lds, want)
        mean = Buf(1, d, d, cuda, dtype=torch.float64)
        p64, p32 = (None if b is None else b.ptr for b in (S64, S32))
        if entry == "shift":
            ws = Ws(lib.deig_syrk_shift_workspace(n, d, xtype), cuda)
            rc = lib.deig_syrk_shift(Xb.ptr, xtype, n, d, ldx, 1.0 / n, p64, lds64, p32, lds, ws.ptr,
                                     ws.nbytes, _stream())
        else:
            ws = Ws(lib.deig_syrk_centered_workspace(n, d, xtype), cuda)
            rc = lib.deig_syrk_centered(Xb.ptr, xtype, n, d, ldx, center.data_ptr(), 1.0 / n, p64, lds64,
                                        p32, lds, mean.ptr, ws.ptr, ws.nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{what} {want}: {L.last_error()}"
        assert Xb.untouched() and ws.canary_intact(), f"{what} {want}"
        for b in (S64, S32):
            assert b is None or b.padding_intact(), f"{what} {want}: wrote outside the result"
        if entry == "centered":
            assert mean.padding_intact()
            np.testing.assert_allclose(mean.numpy()[0], own, rtol=1e-14)
        return S64, S32

    S64, S32 = run(d + 1, d + 1, d + 3, ("S64", "S"))
    got = S64.numpy()
    assert np.isfinite(got).all() and np.isfinite(S32.numpy()).all(), f"{what}: NaN leaked in"
    err = np.abs(got - ref).max()
    print(f"{what}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, f"{what}: max err {err:.3e} > {bar:.3e}"
    assert np.array_equal(got, got.T) and np.array_equal(S32.numpy(), S32.numpy().T), f"{what}: symmetry"
    assert torch.equal(S32.rows(), S64.rows().to(torch.float32)), f"{what}: S is not S64's rounding"
    a64, _ = run(d + 1, d + 1, d + 3, ("S64",))
    _, a32 = run(d + 1, d + 1, d + 3, ("S",))
    assert a64.same_result(S64) and a32.same_result(S32), f"{what}: an output alone differs"
    f64, f32 = run(d, d, d, ("S64", "S"))
    assert S64.same_result(f64) and S32.same_result(f32), f"{what}: differs from the contiguous call"


@pytest.mark.parametrize("mode", ["raw", "gray"])
def test_syrk_u8_padded(mode, cuda):
    """lds = d + 1, lds64 = d + 3, 0xFF bytes behind every row; alpha = 1, so S64 is the
    integer matrix itself (raw) or a ninth of it rounded once (gray), as tests/test_gpu_u8.py
    has it, and S within one fp32 ulp."""
    L = _L()
    lib = L.lib()
    n, d = 300, 260
    rng = np.random.default_rng(n + d)
    code = {"raw": L.DEIG_U8_RAW, "gray": L.DEIG_U8_GRAY3}[mode]
    width = d if mode == "raw" else 3 * d
    X = rng.integers(0, 256, (n, width), dtype=np.uint8)
    if mode == "raw":
        v = X.astype(np.float64)
        ref = v.T @ v
    else:
        s = X.astype(np.float64).reshape(n, d, 3).sum(axis=2)
        ref = (s.T @ s) / 9.0
    what = f"syrk_u8[{mode}]"

    def run(ldx, lds, lds64, want):
        Xb = _inputs(X, ldx, cuda)
        S64, S32 = _cov_outputs(cuda, d, lds64, lds, want)
        p64, p32 = (None if b is None else b.ptr for b in (S64, S32))
        ws = Ws(lib.deig_syrk_u8_workspace(n, d, code), cuda)
        rc = lib.deig_syrk_u8(Xb.ptr, n, d, ldx, code, 1.0, p32, lds, p64, lds64, ws.ptr, ws.nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{what} {want}: {L.last_error()}"
        assert Xb.untouched() and ws.canary_intact(), f"{what} {want}"
        for b in (S64, S32):
            assert b is None or b.padding_intact(), f"{what} {want}: wrote outside the result"
        return S64, S32

    S64, S32 = run(width + 4, d + 1, d + 3, ("S64", "S"))
    g64, g32 = S64.numpy(), S32.numpy().astype(np.float64)
    if mode == "raw":
        np.testing.assert_array_equal(g64, ref)
    else:
        np.testing.assert_allclose(g64, ref, rtol=1e-15, atol=0)
    assert (np.abs(g32 - ref) / np.maximum(np.abs(ref), 1e-30)).max() <= 1.01 * 2.0 ** -23
    assert np.array_equal(g64, g64.T) and np.array_equal(g32, g32.T)
    a64, _ = run(width + 4, d + 1, d + 3, ("S64",))
    _, a32 = run(width + 4, d + 1, d + 3, ("S",))
    assert a64.same_result(S64) and a32.same_result(S32), f"{what}: an output alone differs"
    f64, f32 = run(width, d, d, ("S64", "S"))
    assert S64.same_result(f64) and S32.same_result(f32), f"{what}: differs from the contiguous call"
