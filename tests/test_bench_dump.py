"""bench.py --dump-outputs: the writer of the last timed step's arrays.  CPU only."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_small_arrays_whole_large_ones_sampled(tmp_path):
    g = torch.Generator().manual_seed(3)
    small = torch.randn((70, 33), generator=g, dtype=torch.float64)
    keep = bench.DUMP_MAX_BYTES // 4
    big = torch.randn((3, keep // 2 + 5), generator=g).t()  # non-contiguous, 1.5 x the limit
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"small": small, "big": big})
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("small", "big")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("small", "big")}
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
    assert a["small"].dtype == np.float32 and a["small"].shape == (70, 33)
    np.testing.assert_array_equal(a["small"], small.float().numpy())
    # the sample: float32, at the size limit, entries of the row-major array at positions
    # that depend on its size alone
    assert a["big"].dtype == np.float32 and a["big"].shape == (keep,)
    idx = np.sort(np.random.default_rng(0).integers(0, big.numel(), size=keep))
    np.testing.assert_array_equal(a["big"], big.contiguous().reshape(-1).numpy()[idx])
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])
    assert sum(v.nbytes for v in a.values()) <= 64e6
