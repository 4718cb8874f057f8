"""bench.py --dump-outputs: the writer's formats, its size limit and its fixed sample (no GPU)."""
import os

import numpy as np

import bench


def test_dump_outputs_formats_and_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * 4096)  # 4096 bytes per array
    T = np.arange(64 * 16, dtype=np.float32).reshape(64, 4, 4)  # exactly its share: kept whole
    big = np.arange(1000 * 3, dtype=np.float32).reshape(1000, 3)  # 12000 bytes: sampled rows
    keys = np.array([[1, 2, 2**40 + 1]], dtype=np.uint64)  # 64-bit values stay exact in float64
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"T": T, "big": big, "keys": keys})
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["T", "big", "keys"]
    assert got["T"].dtype == np.float32 and np.array_equal(got["T"], T)
    assert got["keys"].dtype == np.float64 and np.array_equal(got["keys"], keys.astype(np.float64))
    assert got["big"].dtype == np.float32 and got["big"].shape == (4096 // 12, 3)
    rows = (got["big"][:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(got["big"], big[rows])
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))  # the same sample every run


def test_stats_arrays_one_array_per_field():
    st = [dict(iterations=3, inlier_ratio=0.5, overlap_keys=[1, 2, 3]), dict(iterations=4, inlier_ratio=0.25,
                                                                              overlap_keys=[4, 5, 6])]
    a = bench.stats_arrays(st)
    assert a["iterations"].tolist() == [3, 4] and a["overlap_keys"].shape == (2, 3)
    assert bench.stats_arrays([]) == {}
