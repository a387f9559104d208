"""Oja steps about a centre on float32, bfloat16 and uint8 samples taken as they are
(deig_oja_steps_centered, csrc/oja.hip: the two-pass kernels' centred loaders and the uint8
sample type).  A sample is centred where the kernels stage it, t = fl32((double)x - mean) with
one rounding, so the oracle is the float32 two-pass path on the precomputed matrix T of those
values and the kernels must return THE SAME BITS - no tolerance.  ref_cpu.oja_epoch on the
float64 centred samples is the backstop against both being wrong together.

The bytes (mean 128) and the bfloat16 samples (mean 3) taken UNCENTRED at the step size of the
centred ones are not a usable stream: their second moment is dominated by the mean direction
(eigenvalue about m^2 d: eta lambda is about 150 for the bytes at d = 264), the basis'
condition number grows by that factor per batch and the float32 Cholesky-QR of the REFERENCE
itself can break down (NaN columns) where orth_every > 1.  Those cases are still run and must
agree with the reference element for element, NaN where it has NaN; and both sample types are
run uncentred a second time at eta = 1 / (m^2 d) (eta lambda about 1), where the reference must
be finite and every check applies in full."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

P_TOL = 1e-4
# (b, d, k, nb, orth_every) and the sample types that run it
SMALL4 = (7, 4, 2, 2, 1)          # every load clamped to 0
SMALL12 = (50, 12, 3, 3, 2)       # d % 8 == 4: the min(k + 4, d - 4) clamp
ONE = (1, 40, 1, 1, 1)            # b = 1, k = 1
MID = (272, 264, 17, 5, 2)        # empty wave slices, NB = 2
NB3 = (96, 520, 33, 4, 3)         # NB = 3
BIG = (2600, 2816, 64, 2, 1)      # steady loop and tail of both passes, NB = 4
CASES = ([(kind, s) for s in (SMALL4, SMALL12) for kind in ("f32", "u8")]
         + [(kind, s) for s in (ONE, MID, NB3, BIG) for kind in ("f32", "bf16", "u8")])
KINDS = ("f32", "bf16", "u8")


MODES = ("centred", "uncentred")
STABLE = "uncentred-stable-eta"  # uint8 and bfloat16 (a mean far from zero), see the module docstring
MEAN = {"u8": 128.0, "bf16": 3.0}


def _eta(kind, mode="centred", d=0):
    if mode == STABLE:
        return 1.0 / (MEAN[kind] ** 2 * d)
    return 0.02 / 24.0 ** 2 if kind == "u8" else 0.02


def _modes(kind):
    return MODES + (STABLE,) if kind in MEAN else MODES


def _data(nb, b, d, k, seed):
    from distributed_eigenspaces_amd import synthetic
    dev = torch.device("cuda", 0)
    U = synthetic.planted_basis(d, min(k, 16), seed=seed, device=dev)
    X = synthetic.spiked_samples(nb * b, U, seed=seed + 1)
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    V0 = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0]
    return X, V0


def _samples(X, kind):
    if kind == "bf16":  # a mean of about 3: the centre has something to do
        return (X.to(torch.bfloat16) + 3).to(torch.bfloat16)
    if kind == "u8":
        return torch.clip(torch.round(128 + 24 * X), 0, 255).to(torch.uint8)
    return X.float().contiguous()


def _staged(x, c):
    """T: what the kernels stage, as a float32 matrix."""
    return x.float() if c is None else (x.double() - c).float()


def _basis(V0, dev, pad=0, canary=0.0):
    d, k = V0.shape
    buf = torch.full((k, d + pad), canary, dtype=torch.float32, device=dev).t()
    V = buf[:d]
    V.copy_(V0)
    return V, buf, d + pad


def _xtype(x):
    from distributed_eigenspaces_amd import _lib
    return {torch.float32: _lib.DEIG_F32, torch.bfloat16: _lib.DEIG_BF16, torch.uint8: _lib.DEIG_U8}[x.dtype]


def _c_run(x, c, V0, b, nb, orth, eta, *, ref=False, bf16_entry=False, ldx=None, pad=0, canary=0.0,
           fill=0.0):
    """One C call on a workspace of its own; V as numpy.  ref: deig_oja_steps_ex with
    DEIG_OJA_TWO_PASS on the float32 x; bf16_entry: deig_oja_steps_bf16; else
    deig_oja_steps_centered on x (float32 / bfloat16 / uint8) about c (None: NULL)."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    d, k = V0.shape
    nbytes = L.deig_oja_workspace(b, d, k)
    ws = torch.full((nbytes // 4 + 1,), fill, dtype=torch.float32, device=x.device)
    V, buf, ldv = _basis(V0, x.device, pad, canary)
    ldx = x.stride(0) if ldx is None else ldx
    tail = (ctypes.c_float(eta), V.data_ptr(), k, ldv, orth)
    if ref:
        assert x.dtype == torch.float32 and c is None
        rc = L.deig_oja_steps_ex(x.data_ptr(), nb, b, d, ldx, *tail, _lib.DEIG_OJA_TWO_PASS,
                                 ws.data_ptr(), nbytes, None)
    elif bf16_entry:
        assert x.dtype == torch.bfloat16 and c is None
        rc = L.deig_oja_steps_bf16(x.data_ptr(), nb, b, d, ldx, *tail, ws.data_ptr(), nbytes, None)
    else:
        rc = L.deig_oja_steps_centered(x.data_ptr(), _xtype(x), nb, b, d, ldx,
                                       None if c is None else c.data_ptr(), *tail, ws.data_ptr(),
                                       nbytes, None)
    assert rc == _lib.DEIG_OK, _lib.last_error()
    if not ref:  # the call clears the timeout word and never sets it
        assert L.deig_oja_error(ws.data_ptr(), nbytes, b, d, k, None) == _lib.DEIG_OK
    torch.cuda.synchronize()
    out = V.cpu().numpy()
    if pad:
        assert (buf[d:].cpu().numpy() == np.float32(canary)).all(), "rows behind d were touched"
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    """(samples, centre, V0, {mode: reference bits}): computed once per sample type and shape
    and never changed."""
    b, d, k, nb, orth = shape
    X, V0 = _data(nb, b, d, k, seed=b + d + k)
    x = _samples(X, kind)
    c = x.double().mean(0)
    refs = {}
    for mode in _modes(kind):
        cc = c if mode == "centred" else None
        r = _c_run(_staged(x, cc), None, V0, b, nb, orth, _eta(kind, mode, d), ref=True)
        if not (kind in MEAN and mode == "uncentred"):
            assert np.isfinite(r).all(), (kind, shape, mode)
        r.setflags(write=False)
        refs[mode] = r
    return x, c, V0, refs


def _py_basis(V0, dev):
    return V0.float().to(dev).t().contiguous().t()


@pytest.mark.parametrize("kind,shape,mode", [(kd, s, m) for kd, s in CASES for m in _modes(kd)], ids=str)
def test_bits_of_the_two_pass_on_the_staged_matrix(kind, shape, mode, cuda):
    b, d, k, nb, orth = shape
    x, c, V0, refs = _case(kind, shape)
    ref = refs[mode]
    V = _c_run(x, c if mode == "centred" else None, V0, b, nb, orth, _eta(kind, mode, d))
    if np.isfinite(ref).all():
        assert np.isfinite(V).all()
        assert np.array_equal(V, ref)
        Vd = V.astype(np.float64)
        np.testing.assert_allclose(Vd.T @ Vd, np.eye(k), atol=1e-5)
    else:  # a large mean taken uncentred at the centred step size: the reference's own CholQR broke down
        assert kind in MEAN and mode == "uncentred"
        print(f"{kind} {shape} {mode}: the float32 two-pass reference has "
              f"{int((~np.isfinite(ref)).sum())} non-finite entries")
        assert np.array_equal(V, ref, equal_nan=True)


@pytest.mark.parametrize("shape", [ONE, MID, NB3, BIG], ids=str)
def test_uncentred_bf16_is_the_bf16_entry_point(shape, cuda):
    b, d, k, nb, orth = shape
    x, _, V0, refs = _case("bf16", shape)
    for mode in ("uncentred", STABLE):
        eta = _eta("bf16", mode, d)
        V = _c_run(x, None, V0, b, nb, orth, eta, bf16_entry=True)
        assert mode == "uncentred" or np.isfinite(V).all()
        assert np.array_equal(V, refs[mode], equal_nan=True)
        assert np.array_equal(_c_run(x, None, V0, b, nb, orth, eta), V, equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in (ONE, MID, NB3, BIG) if s[2] <= 32 and s[1] >= 264], ids=str)
def test_oracle_backstop(kind, shape, cuda):
    b, d, k, nb, orth = shape
    x, c, V0, _ = _case(kind, shape)
    V = _c_run(x, c, V0, b, nb, orth, _eta(kind)).astype(np.float64)
    xd = x.double()
    Vo = ref_cpu.oja_epoch((xd - c).cpu().numpy(), V0.numpy(), _eta(kind), b)
    dist = ref_cpu.projector_distance(V, Vo)
    print(f"{kind} {shape}: projector distance to ref_cpu.oja_epoch on the centred samples {dist:.3e}")
    assert dist <= P_TOL
    if kind == "u8":  # the test cannot pass by ignoring the centre
        Vu = ref_cpu.oja_epoch(xd.cpu().numpy(), V0.numpy(), _eta(kind), b)
        far = ref_cpu.projector_distance(V, Vu)
        print(f"{kind} {shape}: distance to the uncentred float64 run {far:.3e}")
        assert far > 0.5


@pytest.mark.parametrize("kind,shape", [(kd, MID) for kd in KINDS] + [("f32", SMALL12), ("u8", SMALL12)],
                         ids=str)
def test_nothing_outside_is_read_or_written(kind, shape, cuda):
    b, d, k, nb, orth = shape
    x, c, V0, refs = _case(kind, shape)
    ref_c = refs["centred"]
    extra = {"f32": 4, "bf16": 8, "u8": 4}[kind]
    if kind == "u8":
        wide = torch.full((nb * b, d + extra), 255, dtype=torch.uint8, device=x.device)
    else:
        wide = torch.full((nb * b, d + extra), float("nan"), dtype=x.dtype, device=x.device)
    wide[:, :d] = x
    long_c = torch.full((d + 9,), float("nan"), dtype=torch.float64, device=x.device)
    cv = long_c[1:d + 1]  # 8-byte, not 16-byte aligned; NaN on both sides
    cv.copy_(c)
    V = _c_run(wide[:, :d], cv, V0, b, nb, orth, _eta(kind), ldx=d + extra, pad=3, canary=-7.25)
    assert np.array_equal(V, ref_c)


@pytest.mark.parametrize("kind,shape", [("u8", BIG), ("u8", MID), ("bf16", MID), ("f32", MID)], ids=str)
def test_deterministic_and_poisoned_workspace(kind, shape, cuda):
    """Bit-identical on a repeat, and everything read from the workspace was written first
    (a NaN-filled workspace changes nothing); _c_run checks deig_oja_error == DEIG_OK."""
    b, d, k, nb, orth = shape
    x, c, V0, refs = _case(kind, shape)
    ref_c = refs["centred"]
    outs = [_c_run(x, c, V0, b, nb, orth, _eta(kind), fill=f) for f in (0.0, float("nan"), float("nan"))]
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    assert np.array_equal(outs[0], ref_c)


@pytest.mark.parametrize("kind", KINDS)
def test_python_matches_the_c_calls(kind, cuda):
    import distributed_eigenspaces_amd as de
    b, d, k, nb, orth = MID
    x, c, V0, refs = _case(kind, MID)
    ref_c = refs["centred"]
    eta = _eta(kind)
    V = _py_basis(V0, x.device)
    assert de.oja_steps(x, V, eta, b, orth, center=c) is V
    assert np.array_equal(V.cpu().numpy(), ref_c)
    # a host centre is moved to the device
    V = _py_basis(V0, x.device)
    de.oja_steps(x, V, eta, b, orth, algo="two_pass", check=False, center=c.cpu())
    assert np.array_equal(V.cpu().numpy(), ref_c)
    # oja_step in a loop: one C call per batch, each ending in CholQR2
    V = _py_basis(V0, x.device)
    Vw = V0
    T = _staged(x, c)
    for i in range(nb):
        assert de.oja_step(x[i * b:(i + 1) * b], V, eta, center=c) is V
        Vw = torch.from_numpy(_c_run(T[i * b:(i + 1) * b], None, Vw, b, 1, 1, eta, ref=True).astype(np.float64))
    assert np.array_equal(V.cpu().numpy(), Vw.numpy().astype(np.float32))


@pytest.mark.parametrize("kind", KINDS)
def test_python_padded_copy_of_the_same_dtype(kind, cuda):
    """d = 10 cannot be read in place: the call equals the one on zero-padded samples, centre
    and basis (a padded column stages fl32(0 - 0) = 0)."""
    import distributed_eigenspaces_amd as de
    b, d, k, nb, orth = 50, 10, 3, 3, 2
    X, V0 = _data(nb, b, d, k, seed=11)
    x = _samples(X, kind)
    c = x.double().mean(0)
    dp = 16 if kind == "bf16" else 12
    xp = torch.zeros((nb * b, dp), dtype=x.dtype, device=x.device)
    xp[:, :d] = x
    cp = torch.cat([c, c.new_zeros(dp - d)])
    V0p = torch.cat([V0, V0.new_zeros(dp - d, k)])
    want = _c_run(xp, cp, V0p, b, nb, orth, _eta(kind))
    assert np.isfinite(want).all() and (want[d:] == 0).all()
    V = _py_basis(V0, x.device)
    de.oja_steps(x, V, _eta(kind), b, orth, center=c)
    assert np.array_equal(V.cpu().numpy(), want[:d])


def test_python_resident_with_a_centre_raises(cuda):
    import distributed_eigenspaces_amd as de
    x, c, V0, _ = _case("f32", MID)
    with pytest.raises(ValueError, match="resident"):
        de.oja_steps(x, _py_basis(V0, x.device), 0.02, MID[0], MID[4], algo="resident", center=c)


def test_python_uint8_without_a_centre(cuda):
    import distributed_eigenspaces_amd as de
    # the resident-eligible shape keeps today's route under "auto": widen, the library chooses
    shape = (4096, 1024, 32, 2, 8)
    b, d, k, nb, orth = shape
    X, V0 = _data(nb, b, d, k, seed=b + d + k)
    x = _samples(X, "u8")
    eta = _eta("u8", STABLE, d)
    Va, Vb = _py_basis(V0, x.device), _py_basis(V0, x.device)
    de.oja_steps(x, Va, eta, b, orth, algo="auto")
    de.oja_steps(x.float(), Vb, eta, b, orth, algo="auto")
    assert torch.isfinite(Va).all() and torch.equal(Va, Vb)
    # everywhere else "auto" and "two_pass" read the bytes: the bits of the widened two-pass route
    b, d, k, nb, orth = MID
    x, _, V0, refs = _case("u8", MID)
    eta, ref_u = _eta("u8", STABLE, d), refs[STABLE]
    for algo in ("auto", "two_pass"):
        Va, Vb = _py_basis(V0, x.device), _py_basis(V0, x.device)
        de.oja_steps(x, Va, eta, b, orth, algo=algo)
        de.oja_steps(x.float(), Vb, eta, b, orth, algo="two_pass")
        assert torch.isfinite(Va).all() and torch.equal(Va, Vb)
        assert np.array_equal(Va.cpu().numpy(), ref_u)


def test_no_float32_copy(cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd import _lib
    shape = (256, 512, 16, 16, 8)
    b, d, k, nb, orth = shape
    x, c, V0, refs = _case("u8", shape)
    ref_c = refs["centred"]
    eta = _eta("u8")
    n = nb * b
    V = _py_basis(V0, x.device)
    de.oja_steps(x, V, eta, b, orth, center=c)  # warm-up: allocates the cached workspace
    torch.cuda.synchronize()
    assert _lib.lib().deig_oja_workspace(b, d, k) <= n * d  # so that the bound below means something
    V.copy_(V0)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    de.oja_steps(x, V, eta, b, orth, center=c)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes; a float32 copy is {n * d * 4}")
    assert rise < n * d * 4
    assert np.array_equal(V.cpu().numpy(), ref_c)


@pytest.mark.parametrize("kind", ["u8", "bf16"])
def test_streaming_fixed_centre(kind, cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd.streaming import StreamingOja
    b, d, k, nb, orth = MID
    x, c, V0, refs = _case(kind, MID)
    ref_c = refs["centred"]
    eta = _eta(kind)
    V0d = V0.float().to(x.device)
    est = StreamingOja(V0d, eta, agg_every=0, center=c)
    assert torch.equal(est.mean_, c)
    V = _py_basis(V0, x.device)
    for i in range(nb):
        est.partial_fit(x[i * b:(i + 1) * b])
        de.oja_step(x[i * b:(i + 1) * b], V, eta, center=c)
        assert torch.isfinite(est.V).all() and torch.equal(est.V, V)
    est = StreamingOja(V0d, eta, agg_every=0, center=c)
    est.partial_fit_block(x, b, orth)
    assert np.array_equal(est.V.cpu().numpy(), ref_c)
    assert est.batches_seen == nb


@pytest.mark.parametrize("kind", ["u8", "bf16"])
def test_streaming_running_centre(kind, cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd.streaming import StreamingOja
    b, d, k, nb, orth = MID
    x, _, V0, _ = _case(kind, MID)
    eta = _eta(kind)
    est = StreamingOja(V0.float().to(x.device), eta, agg_every=0, center="running")
    assert est.mean_ is None
    V = _py_basis(V0, x.device)
    for i in range(nb):
        est.partial_fit(x[i * b:(i + 1) * b])
        want = x[:(i + 1) * b].double().cpu().numpy().mean(0)
        np.testing.assert_allclose(est.mean_.cpu().numpy(), want, rtol=1e-12, atol=0)
        de.oja_step(x[i * b:(i + 1) * b], V, eta, center=est.mean_)
        assert torch.isfinite(est.V).all() and torch.equal(est.V, V)
    # a block: the mean takes the whole segment in before its steps
    est = StreamingOja(V0.float().to(x.device), eta, agg_every=0, center="running")
    est.partial_fit_block(x, b, orth)
    np.testing.assert_allclose(est.mean_.cpu().numpy(), x.double().cpu().numpy().mean(0), rtol=1e-12, atol=0)
    V = _py_basis(V0, x.device)
    de.oja_steps(x, V, eta, b, orth, center=est.mean_)
    assert torch.equal(est.V, V)


@pytest.mark.parametrize("kind", KINDS)
def test_streaming_without_a_centre_is_unchanged(kind, cuda):
    from distributed_eigenspaces_amd.streaming import StreamingOja
    b, d, k, nb, orth = MID
    x, _, V0, _ = _case(kind, MID)
    eta = _eta(kind, STABLE, d) if kind in MEAN else _eta(kind)  # uncentred: see the module docstring
    V0d = V0.float().to(x.device)
    sa, sb = StreamingOja(V0d, eta, agg_every=0, center=None), StreamingOja(V0d, eta, agg_every=0)
    assert sa.mean_ is None
    for i in range(nb):
        sa.partial_fit(x[i * b:(i + 1) * b])
        sb.partial_fit(x[i * b:(i + 1) * b])
        assert torch.isfinite(sa.V).all() and torch.equal(sa.V, sb.V)
    sa.partial_fit_block(x, b, orth)
    sb.partial_fit_block(x, b, orth)
    assert torch.isfinite(sa.V).all() and torch.equal(sa.V, sb.V)
