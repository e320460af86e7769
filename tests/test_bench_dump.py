"""bench.py --dump-outputs on host tensors: names, dtypes, the 64 MB bound and the fixed seeded sample of large outputs."""

import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_float_arrays_within_the_bound_and_samples_large_ones_the_same_way(tmp_path):
    big = torch.arange(3 * bench.DUMP_MAX_ELEMS, dtype=torch.float64).reshape(3, -1)
    params = [torch.randn(bench.DUMP_WEIGHT_ELEMS, generator=torch.Generator().manual_seed(0)), torch.ones(7, 5)]
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), {"sample": big, "train_loss": torch.tensor(0.25, dtype=torch.float16)}, params)
    assert sorted(os.listdir(tmp_path / "a")) == ["sample.npy", "train_loss.npy", "weights_sample.npy"]
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES
    assert a["sample"].dtype == np.float64 and a["sample"].shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(a["sample"]) >= 0) and np.all(a["sample"] == np.round(a["sample"]))   # entries of the output, in order
    assert a["train_loss"].dtype == np.float32 and a["train_loss"] == 0.25
    assert a["weights_sample"].dtype == np.float32 and a["weights_sample"].shape == (bench.DUMP_WEIGHT_ELEMS,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_keeps_small_outputs_whole(tmp_path):
    x = torch.randn(2, 3, 16, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), {"sample": x})
    assert os.listdir(tmp_path) == ["sample.npy"]
    assert np.array_equal(np.load(tmp_path / "sample.npy"), x.numpy())
