"""Leading-dimension and alignment rules of the solver-era entry points that the library
rejects up front (include/deig.h): each call below breaks exactly one of them and must come
back DEIG_EINVAL with a message that names the rule, before any GPU work - the operands are
made-up addresses that nothing may look at, so this runs on a machine without a GPU (CPU).

The rules: the projector average with k > 128 deflates its locked blocks by products with V
itself and needs a 16-byte aligned V with ldv % 4 == 0; the fp32 solver takes a float32 S
only; the fp32 sweep needs a 16-byte aligned Q with ldq % 4 == 0; the fused power chain needs
that of Q and Y both."""
import ctypes

import pytest

from distributed_eigenspaces_amd import _lib

# made-up, 256-byte aligned "device" addresses
S_, V_, E_, Q_, Y_, W_, WS_, CS_ = (0x10000 * (i + 1) for i in range(8))
F = ctypes.c_float


def _einval(rc, *words):
    assert rc == _lib.DEIG_EINVAL, (rc, _lib.last_error())
    msg = _lib.last_error()
    assert msg, "no message"
    for w in words:
        assert w in msg, (w, msg)


def _topk(d, k, ldv, V=V_, stype=None, lds=None, **opts):
    o = _lib.solver_opts(**opts)
    return _lib.lib().deig_topk_sym_ex(S_, _lib.DEIG_F32 if stype is None else stype, d, lds or d, k, 0,
                                       100, F(1e-6), None, 0, 0, V, ldv, E_, None, None,
                                       ctypes.byref(o), WS_, 1 << 30, None)


def test_fp32_solver_rejects_float64_matrix():
    """sweep_algo = DEIG_SWEEP_FP32 reads S itself on the f32 MFMA: a float64 S is refused
    by the wrapper (it used to be refused after the first problems of a batch were staged)."""
    for ldv in (256, 257):
        _einval(_topk(256, 8, ldv, stype=_lib.DEIG_F64, sweep_algo=_lib.DEIG_SWEEP_FP32), "topk",
                "float64")
    W = 3
    o = _lib.solver_opts(sweep_algo=_lib.DEIG_SWEEP_FP32)
    S = (ctypes.c_void_p * W)(*[S_ + 0x1000 * i for i in range(W)])
    V = (ctypes.c_void_p * W)(*[V_ + 0x1000 * i for i in range(W)])
    E = (ctypes.c_void_p * W)(*[E_ + 0x100 * i for i in range(W)])
    status = (ctypes.c_int * W)(7, 7, 7)
    rc = _lib.lib().deig_topk_sym_batch_ex(W, S, _lib.DEIG_F64, 256, 256, 8, 0, 100, F(1e-6), V, 256,
                                           E, None, None, status, ctypes.byref(o), WS_, 1 << 30, None)
    _einval(rc, "topk_batch", "float64")
    assert list(status) == [7, 7, 7], "status written by a call that was rejected"


@pytest.mark.parametrize("ldv,off", [(513, 0), (514, 0), (512, 4)])
def test_projavg_block_locking_rejects_unaligned_basis(ldv, off):
    """k > 128 on the implicit operator: the locked blocks are deflated by products with V."""
    L = _lib.lib()
    d, k, mk = 512, 160, 320
    args = (W_, d, mk, d + 4, F(0.5), k, 0, 100, F(1e-6), None, 0, 0, V_ + off, ldv, E_, None, None)
    _einval(L.deig_projavg_topk_f32(*args, WS_, 1 << 30, None), "projavg", "k > 128", "ldv % 4 == 0")
    o = _lib.solver_opts()
    _einval(L.deig_projavg_topk_ex(*args, ctypes.byref(o), WS_, 1 << 30, None), "projavg", "k > 128",
            "ldv % 4 == 0")


def _apply(algo, d=256, lds=256, p=32, ldq=32, ldy=32, S=S_, Q=Q_, Y=Y_):
    return _lib.lib().deig_sym_apply_f32(S, d, lds, Q, p, ldq, Y, ldy, F(1.0), algo, WS_, 1 << 30, None)


def test_fp32_sweep_operand_rules():
    fp32 = _lib.DEIG_SWEEP_FP32
    for kw in ({"ldq": 33}, {"ldq": 34}, {"ldq": 28}, {"Q": Q_ + 4}, {"Q": None}, {"ldy": 31},
               {"Y": None}):
        _einval(_apply(fp32, **kw), "sym_apply", "DEIG_SWEEP_FP32", "ldq % 4 == 0")
    for kw in ({"lds": 257}, {"lds": 252}, {"S": S_ + 4}, {"S": None}, {"d": 254, "lds": 256}):
        _einval(_apply(fp32, **kw), "sym_apply", "DEIG_SWEEP_FP32", "lds % 4 == 0")


def test_bf16x6_sweep_shape_rules():
    """The bf16x6 sweep takes any ldq, ldy >= p; what it cannot take is rejected before
    the image of S is built."""
    for algo in (_lib.DEIG_SWEEP_AUTO, _lib.DEIG_SWEEP_BF16X6 | _lib.DEIG_SWEEP_ROUND_Q):
        _einval(_apply(algo, ldq=31), "sym_apply", "ldq >= p")
        _einval(_apply(algo, ldy=31), "sym_apply", "ldy >= p")
        _einval(_apply(algo, p=24, ldq=24, ldy=24), "sym_apply", "p=24")
        _einval(_apply(algo, Q=None), "sym_apply", "null")


def _power(p=32, ldq=32, ldy=32, Q=Q_, Y=Y_, algo=None):
    return _lib.lib().deig_sym_power_f32(S_, 256, 256, Q, p, ldq, Y, ldy, CS_, 3,
                                         _lib.DEIG_SWEEP_BF16X6 if algo is None else algo, WS_,
                                         1 << 30, None)


def test_power_chain_operand_rules():
    for kw in ({"ldq": 33}, {"ldq": 35}, {"ldy": 33}, {"ldy": 34}, {"Q": Q_ + 4}, {"Y": Y_ + 8},
               {"ldq": 33, "ldy": 35}):
        _einval(_power(**kw), "sym_power", "ldq % 4 == 0", "ldy % 4 == 0", "16-byte")
    _einval(_power(ldq=28), "sym_power", "ldq >= p")
    _einval(_power(ldy=16), "sym_power", "ldy >= p")
    _einval(_power(p=40, ldq=40, ldy=40), "sym_power", "p=40")
    _einval(_power(Y=None), "sym_power", "null")
    _einval(_power(algo=_lib.DEIG_SWEEP_FP32), "sym_power", "bf16x6")
