"""The sample operator of the covariance-free route, Y = alpha Xc^T (Xc Q) (deig_gram_apply,
csrc/gram.hip), on float32, bfloat16 and uint8 samples, with and without a centre.

The reference is float64 NumPy on the STAGED matrix Xc = fl32((double)x - c), rebuilt here.
The bound is derived, not tuned: a float32 dot product of length m, summed in any order, errs
by at most gamma_m = m u / (1 - m u), u = 2^-24, times the product of absolute values.  Two
chained products (lengths d and n) and the rounding of alpha give, element by element,

    |Y - Y64| <= (gamma_n + gamma_d + gamma_n gamma_d + 2 u) alpha |Xc|^T (|Xc| |Q|)

with the right-hand side in float64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = ((1, 16, 16), (31, 20, 16), (33, 64, 16), (65, 68, 48), (200, 132, 80), (97, 260, 128))
KINDS = ("f32", "bf16", "u8")
NAN_WORD = 0x7FC00000


def _gamma(m):
    return m * U / (1.0 - m * U)


def _dev():
    return torch.device("cuda", 0)


def _xtype(x):
    from distributed_eigenspaces_amd import _lib
    return {torch.float32: _lib.DEIG_F32, torch.bfloat16: _lib.DEIG_BF16, torch.uint8: _lib.DEIG_U8}[x.dtype]


def _d_of(kind, d):
    return (d + 7) // 8 * 8 if kind == "bf16" else d


@functools.lru_cache(maxsize=None)
def _case(kind, n, d, p, centred, seed=0):
    """(x with ldx = d + 8 and poisoned padding, centre or None, Q, Xc float64) on the host."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + d + p)
    ld = d + 8
    if kind == "u8":
        buf = torch.full((n, ld), 255, dtype=torch.uint8)
        buf[:, :d] = torch.randint(0, 256, (n, d), generator=g, dtype=torch.uint8)
        scale, mean = 74.0, 128.0
    else:
        dt = torch.float32 if kind == "f32" else torch.bfloat16
        buf = torch.full((n, ld), float("nan"), dtype=dt)
        buf[:, :d] = (torch.randn(n, d, generator=g) + 0.5).to(dt)
        scale, mean = 1.0, 0.5
    c = (mean + scale * torch.randn(d, generator=g, dtype=torch.float64)) if centred else None
    Q = torch.randn(d, p, generator=g, dtype=torch.float32)
    x64 = buf[:, :d].to(torch.float64)
    Xc = x64 if c is None else (x64 - c).to(torch.float32).to(torch.float64)
    return buf, c, Q, Xc.numpy()


def _run(buf, d, c, Q, alpha, *, ld2=False, ws_rows=None, canary=None):
    """One deig_gram_apply on a workspace of its own, filled with NaN bit patterns."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    dev = _dev()
    x = buf.to(dev)
    n = x.shape[0]
    p = Q.shape[1]
    ldq = 2 * p if ld2 else p
    Qd = torch.full((d, ldq), float("nan"), dtype=torch.float32, device=dev)
    Qd[:, :p] = Q.to(dev)
    Yd = torch.full((d, ldq), -7.0 if canary is None else canary, dtype=torch.float32, device=dev)
    xt = _xtype(x)
    nbytes = L.deig_gram_apply_workspace(n if ws_rows is None else ws_rows, d, p, xt)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 1,), NAN_WORD, dtype=torch.int32, device=dev)
    cd = None if c is None else c.to(dev)
    rc = L.deig_gram_apply(x.data_ptr(), xt, n, d, x.stride(0), None if cd is None else cd.data_ptr(),
                           ctypes.c_float(alpha), Qd.data_ptr(), p, ldq, Yd.data_ptr(), ldq,
                           ws.data_ptr(), nbytes, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    Y = Yd.cpu()
    return Y[:, :p].numpy().copy(), Y[:, p:].numpy().copy()


def _check(Y, Xc, Q, alpha):
    n, d = Xc.shape
    Q64 = Q.to(torch.float64).numpy()
    a = float(np.float32(alpha))
    ref = a * (Xc.T @ (Xc @ Q64))
    bound = (_gamma(n) + _gamma(d) + _gamma(n) * _gamma(d) + 2 * U) * a * (np.abs(Xc).T @ (np.abs(Xc) @ np.abs(Q64)))
    err = np.abs(Y.astype(np.float64) - ref)
    assert np.isfinite(Y).all()
    worst = float((err - bound).max())
    print(f"max err {err.max():.3e}, max bound {bound.max():.3e}, worst margin {worst:.3e}")
    assert (err <= bound).all(), f"error exceeds the derived bound by {worst:.3e}"


@pytest.mark.parametrize("centred", (False, True), ids=("uncentred", "centred"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_gram_apply_meets_the_derived_bound(kind, shape, centred):
    n, d, p = shape
    d = _d_of(kind, d)
    buf, c, Q, Xc = _case(kind, n, d, p, centred)
    alpha = 1.0 / n
    Y, _ = _run(buf, d, c, Q, alpha)
    _check(Y, Xc, Q, alpha)
    # ldq = ldy = 2 p: the same bits, and nothing behind column p of a Y row is written
    Y2, tail = _run(buf, d, c, Q, alpha, ld2=True, canary=12345.0)
    assert np.array_equal(Y, Y2)
    assert (tail == 12345.0).all()
    # repeated calls give identical bits
    Y3, _ = _run(buf, d, c, Q, alpha)
    assert np.array_equal(Y, Y3)


@pytest.mark.parametrize("kind", KINDS)
def test_gram_apply_integers_are_exact(kind):
    """Integer X and Q with partial sums below 2^24, alpha = 1, no centre: the exact result."""
    n, d, p = 70, 136, 32
    g = torch.Generator().manual_seed(5)
    xi = torch.randint(0, 8, (n, d), generator=g)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[kind]
    Q = torch.randint(-3, 4, (d, p), generator=g).to(torch.float32)
    # |Xc Q| <= 136 * 7 * 3 < 2^12, |Y| <= 70 * 7 * 2^12 < 2^21
    Y, _ = _run(xi.to(dt), d, None, Q, 1.0)
    X64 = xi.to(torch.float64).numpy()
    assert np.array_equal(Y.astype(np.float64), X64.T @ (X64 @ Q.to(torch.float64).numpy()))


@pytest.mark.parametrize("centred", (False, True), ids=("uncentred", "centred"))
@pytest.mark.parametrize("kind", KINDS)
def test_gram_apply_row_chunks(kind, centred):
    """n = 5000 with the workspace of 1700 rows: three chunks, added in chunk order - the same
    bound, and the same bits on a second call."""
    n, d, p = 5000, 136 if kind == "bf16" else 132, 32
    buf, c, Q, Xc = _case(kind, n, d, p, centred, seed=3)
    alpha = 1.0 / n
    Y, _ = _run(buf, d, c, Q, alpha, ws_rows=1700)
    _check(Y, Xc, Q, alpha)
    Y2, _ = _run(buf, d, c, Q, alpha, ws_rows=1700)
    assert np.array_equal(Y, Y2)


def test_gram_apply_python_op():
    """linalg.gram_apply: samples read in place, and a view that is copied (d % 4 != 0)."""
    import distributed_eigenspaces_amd as de
    buf, c, Q, Xc = _case("f32", 200, 132, 80, True)
    x = buf.to(_dev())[:, :132]
    Y = de.gram_apply(x, Q.to(_dev()), center=c)
    _check(Y.cpu().numpy(), Xc, Q, 1.0 / 200)
    xo = x[:, :130]
    Yo = de.gram_apply(xo, Q[:130].to(_dev()), center=c[:130])
    assert Yo.shape == (130, 80)
    _check(Yo.cpu().numpy(), Xc[:, :130], Q[:130], 1.0 / 200)
    with pytest.raises(TypeError, match="explicit route"):
        de.gram_apply(x.double(), Q.to(_dev()))
