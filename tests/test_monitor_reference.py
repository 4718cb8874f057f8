"""The monitor's restatement (tests/monitor_reference.py) against an independent brute force: numpy
all-pairs distances in float64 (and scipy's cKDTree where it is installed) on small clouds, and its
quantile indices. No device."""
import numpy as np
import pytest

import monitor_reference as mr


def brute_d2(tree_pts, queries):
    """float64 squared distance of every query to its nearest tree point."""
    a = np.asarray(queries, np.float64)[:, None, :3]
    b = np.asarray(tree_pts, np.float64)[None, :, :3]
    return ((a - b) ** 2).sum(-1).min(1)


def clouds(seed, n_ref, n_out):
    rng = np.random.default_rng(seed)
    return ((rng.random((n_ref, 3)) * 4).astype(np.float32), (rng.random((n_out, 3)) * 4).astype(np.float32))


@pytest.mark.parametrize("n,q,index", [(5, 0.6, 3), (10, 0.7, 7), (5, 0.0, 0), (10, 0.0, 0), (5, 1.0, 4), (10, 1.0, 9),
                                        (5, 0.7, 3), (10, 0.6, 6)])
def test_quantile_indices(oracle, n, q, index):
    """values[(size_t)((float)n * q)]: float(5) * 0.6f = 3.0000002 -> 3, float(10) * 0.7f = 6.9999998
    in exact arithmetic but 7 as a float product; q == 1 is the maximum."""
    assert mr.quantile_index(n, q) == index
    v = np.random.default_rng(n).permutation(n).astype(np.float32) + 1
    got, err = oracle.dists_quantile(v, float(np.float32(q)))
    assert err == 0 and got == np.sort(v)[index]


@pytest.mark.parametrize("seed,n_ref,n_out", [(1, 1, 1), (2, 1, 40), (3, 300, 257), (4, 500, 700)])
def test_restatement_against_brute_force(oracle, seed, n_ref, n_out):
    ref, out = clouds(seed, n_ref, n_out)
    r = mr.monitor(oracle, ref, out, quantile=0.6, max_accepted_dist=0.2)
    b = [brute_d2(ref, out), brute_d2(out, ref)]
    # float d2 of three rounded squares of rounded differences: a few ulps of the largest term
    for got, want in zip((r["d2_out"], r["d2_ref"]), b):
        assert np.allclose(got, want, rtol=1e-5, atol=1e-9)
    assert np.isclose(float(r["hausdorff"]), np.sqrt(max(b[0].max(), b[1].max())), rtol=1e-5)
    for k in range(2):
        assert r["max_d2"][k] == r["d2_out" if k == 0 else "d2_ref"].max()
        d = np.sort(r["d2_out" if k == 0 else "d2_ref"])
        assert r["quantile_d2"][k] == d[mr.quantile_index(len(d), 0.6)]
    assert r["hausdorff_quantile"] == np.sqrt(max(r["quantile_d2"]))
    # validity away from the 0.2 m boundary only: both sides round differently next to it
    db = np.sqrt(b[0])
    clear = np.abs(db - 0.2) > 1e-5
    assert np.array_equal((r["dist_out"].astype(np.float64) <= 0.2)[clear], (db <= 0.2)[clear])
    if clear.all() and (db <= 0.2).any():
        assert r["knn_valid"] == int((db <= 0.2).sum())
        assert np.isclose(float(r["knn_mean_dist"]), db[db <= 0.2].mean(), rtol=1e-5)
    if not (db <= 0.2 + 1e-5).any():
        assert r["knn_valid"] == 0 and np.isnan(r["knn_mean_dist"])


def test_restatement_paired_exact_search_is_direction_zero(oracle):
    """epsilon 0 in a bucket-8 tree without a radius: the trimmed filter runs on direction 0."""
    ref, out = clouds(7, 400, 333)

    class Cfg:
        nn_epsilon, nn_max_dist, trimmed_ratio, bucket_size = 0.0, float("inf"), 0.7, 8

    r = mr.monitor(oracle, ref, out, cfg=Cfg)
    d = np.sort(r["d2_out"])
    lim = d[mr.quantile_index(len(d), 0.7)]
    assert r["paired_limit_d2"] == lim and r["paired_kept"] == int((r["d2_out"] <= lim).sum())
    b = np.sqrt(brute_d2(ref, out))
    assert np.isclose(float(r["paired_mean_dist"]), np.sort(b)[: r["paired_kept"]].mean(), rtol=1e-5)


def test_restatement_against_ckdtree(oracle):
    sp = pytest.importorskip("scipy.spatial")
    ref, out = clouds(9, 2000, 1500)
    r = mr.monitor(oracle, ref, out)
    d, _ = sp.cKDTree(ref.astype(np.float64)).query(out.astype(np.float64))
    assert np.allclose(r["dist_out"], d, rtol=1e-5, atol=1e-7)
    d, _ = sp.cKDTree(out.astype(np.float64)).query(ref.astype(np.float64))
    assert np.allclose(r["dist_ref"], d, rtol=1e-5, atol=1e-7)


def test_restatement_transform_and_empty_valid_set(oracle):
    ref, out = clouds(11, 200, 200)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [5.0, 0.0, 0.0]   # a 4 m cube moved by 5 m: nothing within 0.2 m
    r = mr.monitor(oracle, ref, out, T=T)
    moved = mr.monitor(oracle, ref, oracle.transform_cloud(T, out))
    assert r["knn_valid"] == 0 and np.isnan(r["knn_mean_dist"])
    assert np.array_equal(r["d2_out"], moved["d2_out"]) and r["hausdorff"] == moved["hausdorff"]
