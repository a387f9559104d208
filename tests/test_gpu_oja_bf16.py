"""Oja steps on bfloat16 samples taken as they are (deig_oja_steps_bf16, csrc/oja.hip: the
two-pass kernels instantiated on the sample type, two MFMAs per fragment pair).  The oracle
is the float32 two-pass path on the widened samples: a bf16 value is its own hi piece and
its lo piece is exactly zero, so the bf16 kernels must return THE SAME BITS - no tolerance.
ref_cpu.oja_epoch is the backstop against both being wrong together."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

P_TOL = 1e-4
ETA = 0.02
# (b, d, k, nb, orth_every): the smallest shapes that reach each branch of the two passes
SHAPES = [
    (50, 8, 3, 3, 2),         # one clamped k-step; b no multiple of 16 or 32
    (1, 40, 1, 1, 1),         # b = 1, k = 1; a full plus a partial k-step
    (272, 264, 17, 5, 2),     # nks = 9: per = 2, waves 5-7 have empty slices; NB = 2
    (96, 520, 33, 4, 3),      # NB = 3
    (2600, 2816, 64, 2, 1),   # 11 k-steps per wave in both passes: steady loop and tail; NB = 4
    (4096, 1024, 32, 2, 8),   # a resident-eligible shape: the entry point still runs two-pass
]
MID = (272, 264, 17, 5, 2)
BIG = (2600, 2816, 64, 2, 1)


def _data(nb, b, d, k, seed):
    from distributed_eigenspaces_amd import synthetic
    dev = torch.device("cuda", 0)
    U = synthetic.planted_basis(d, min(k, 16), seed=seed, device=dev)
    X = synthetic.spiked_samples(nb * b, U, seed=seed + 1)
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    V0 = torch.linalg.qr(torch.randn(d, k, generator=g, dtype=torch.float64))[0]
    return X, V0


def _basis(V0, dev, pad=0, canary=0.0):
    """V0 as a (d, k) column-major float32 device tensor with ldv = d + pad (the rows
    behind d hold the canary); returns (V, its buffer, ldv)."""
    d, k = V0.shape
    buf = torch.full((k, d + pad), canary, dtype=torch.float32, device=dev).t()
    V = buf[:d]
    V.copy_(V0)
    return V, buf, d + pad


def _c_run(X, V0, b, nb, orth, *, ldx=None, pad=0, canary=0.0, fill=0.0, check_err=False):
    """One call of the C entry point of X's dtype (bf16: deig_oja_steps_bf16; float32:
    deig_oja_steps_ex with DEIG_OJA_TWO_PASS) on a workspace of its own; V as numpy."""
    from distributed_eigenspaces_amd import _lib
    L = _lib.lib()
    d, k = V0.shape
    nbytes = L.deig_oja_workspace(b, d, k)
    ws = torch.full((nbytes // 4 + 1,), fill, dtype=torch.float32, device=X.device)
    V, buf, ldv = _basis(V0, X.device, pad, canary)
    ldx = X.stride(0) if ldx is None else ldx
    head = (X.data_ptr(), nb, b, d, ldx, ctypes.c_float(ETA), V.data_ptr(), k, ldv, orth)
    if X.dtype == torch.bfloat16:
        rc = L.deig_oja_steps_bf16(*head, ws.data_ptr(), nbytes, None)
    else:
        rc = L.deig_oja_steps_ex(*head, _lib.DEIG_OJA_TWO_PASS, ws.data_ptr(), nbytes, None)
    assert rc == _lib.DEIG_OK, _lib.last_error()
    if check_err:  # the bf16 path clears the timeout word and never sets it
        assert L.deig_oja_error(ws.data_ptr(), nbytes, b, d, k, None) == _lib.DEIG_OK
    torch.cuda.synchronize()
    out = V.cpu().numpy()
    if pad:
        assert (buf[d:].cpu().numpy() == np.float32(canary)).all(), "rows behind d were touched"
    return out


@functools.lru_cache(maxsize=None)
def _case(b, d, k, nb, orth):
    """(bf16 samples, V0, reference bits): computed once per shape and never changed."""
    X, V0 = _data(nb, b, d, k, seed=b + d + k)
    x16 = X.to(torch.bfloat16)
    ref = _c_run(x16.float(), V0, b, nb, orth)
    assert np.isfinite(ref).all()
    ref.setflags(write=False)
    return x16, V0, ref


def _py_basis(V0, dev):
    return V0.float().to(dev).t().contiguous().t()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bits_of_the_widened_two_pass(shape, cuda):
    b, d, k, nb, orth = shape
    x16, V0, ref = _case(*shape)
    V = _c_run(x16, V0, b, nb, orth, check_err=True)
    assert np.isfinite(V).all()
    assert np.array_equal(V, ref)
    Vd = V.astype(np.float64)
    np.testing.assert_allclose(Vd.T @ Vd, np.eye(k), atol=1e-5)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] <= 32 and s[1] >= 264], ids=str)
def test_oracle_backstop(shape, cuda):
    b, d, k, nb, orth = shape
    x16, V0, _ = _case(*shape)
    V = _c_run(x16, V0, b, nb, orth).astype(np.float64)
    Vo = ref_cpu.oja_epoch(x16.double().cpu().numpy(), V0.numpy(), ETA, b)
    dist = ref_cpu.projector_distance(V, Vo)
    print(f"{shape}: projector distance to ref_cpu.oja_epoch {dist:.3e}")
    assert dist <= P_TOL


def test_padding_is_never_read(cuda):
    import distributed_eigenspaces_amd as de
    b, d, k, nb, orth = MID
    x16, V0, ref = _case(*MID)
    wide = torch.full((nb * b, d + 8), float("nan"), dtype=torch.bfloat16, device=x16.device)
    wide[:, :d] = x16
    view = wide[:, :d]
    assert np.array_equal(_c_run(view, V0, b, nb, orth, ldx=d + 8), ref)
    V = _py_basis(V0, x16.device)
    de.oja_steps(view, V, ETA, b, orth, algo="two_pass")
    assert np.array_equal(V.cpu().numpy(), ref)


def test_padded_column_major_basis(cuda):
    b, d, k, nb, orth = MID
    x16, V0, ref = _case(*MID)
    V = _c_run(x16, V0, b, nb, orth, pad=3, canary=-7.25)  # checks the canary itself
    assert np.array_equal(V, ref)


def test_deterministic_and_poisoned_workspace(cuda):
    """Bit-identical on a repeat, and everything read from the workspace was written first
    (a NaN-filled workspace changes nothing)."""
    b, d, k, nb, orth = BIG
    x16, V0, ref = _case(*BIG)
    outs = [_c_run(x16, V0, b, nb, orth, fill=f) for f in (0.0, float("nan"), float("nan"))]
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    assert np.array_equal(outs[0], ref)


def test_python_routing(cuda):
    import distributed_eigenspaces_amd as de
    b, d, k, nb, orth = MID
    x16, V0, ref = _case(*MID)
    dev = x16.device
    V = _py_basis(V0, dev)
    assert de.oja_steps(x16, V, ETA, b, orth, algo="two_pass") is V
    assert np.array_equal(V.cpu().numpy(), ref)
    # oja_step in a loop: one C call per batch, each ending in CholQR2
    V = _py_basis(V0, dev)
    Vw = V0
    for i in range(nb):
        de.oja_step(x16[i * b:(i + 1) * b], V, ETA)
        Vw = torch.from_numpy(_c_run(x16[i * b:(i + 1) * b].float(), Vw, b, 1, 1).astype(np.float64))
    assert np.array_equal(V.cpu().numpy(), Vw.numpy().astype(np.float32))


def test_fallbacks_keep_the_float32_route(cuda):
    import distributed_eigenspaces_amd as de
    # d = 12 (d % 8 == 4): widened, as before
    X, V0 = _data(3, 50, 12, 3, seed=5)
    x16 = X.to(torch.bfloat16)
    Va, Vb = _py_basis(V0, X.device), _py_basis(V0, X.device)
    de.oja_steps(x16, Va, ETA, 50, 2)
    de.oja_steps(x16.float(), Vb, ETA, 50, 2)
    assert torch.isfinite(Va).all() and torch.equal(Va, Vb)
    # algo="resident" on bf16: the resident kernel on the widened samples, as before
    shape = (4096, 1024, 32, 2, 8)
    b, d, k, nb, orth = shape
    x16, V0, _ = _case(*shape)
    Va, Vb = _py_basis(V0, x16.device), _py_basis(V0, x16.device)
    de.oja_steps(x16, Va, ETA, b, orth, algo="resident")
    de.oja_steps(x16.float(), Vb, ETA, b, orth, algo="resident")
    assert torch.isfinite(Va).all() and torch.equal(Va, Vb)


def test_no_float32_copy(cuda):
    import distributed_eigenspaces_amd as de
    from distributed_eigenspaces_amd import _lib
    shape = (256, 512, 16, 16, 8)
    b, d, k, nb, orth = shape
    x16, V0, ref = _case(*shape)
    n = nb * b
    V = _py_basis(V0, x16.device)
    de.oja_steps(x16, V, ETA, b, orth)  # warm-up: allocates the cached workspace
    torch.cuda.synchronize()
    assert _lib.lib().deig_oja_workspace(b, d, k) <= n * d  # so that the bound below means something
    V.copy_(V0)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    de.oja_steps(x16, V, ETA, b, orth)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes; a float32 copy is {n * d * 4}")
    assert rise < n * d * 4
    assert np.array_equal(V.cpu().numpy(), ref)


def test_streaming_oja_takes_bf16(cuda):
    from distributed_eigenspaces_amd.streaming import StreamingOja
    b, d, k, nb, orth = MID
    x16, V0, _ = _case(*MID)
    V0d = V0.float().to(x16.device)
    s16, s32 = StreamingOja(V0d, ETA, agg_every=0), StreamingOja(V0d, ETA, agg_every=0)
    for i in range(nb):
        blk = x16[i * b:(i + 1) * b]
        s16.partial_fit(blk)
        s32.partial_fit(blk.float())
        assert torch.isfinite(s16.V).all() and torch.equal(s16.V, s32.V)
    s16.partial_fit_block(x16, b, orth)
    s32.partial_fit_block(x16.float(), b, orth)
    assert torch.isfinite(s16.V).all() and torch.equal(s16.V, s32.V)
    assert s16.batches_seen == 2 * nb
