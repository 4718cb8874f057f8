"""The sampled chains' filters on the device (aicp_hip_chain_filter) against
chain_reference: the compaction's edges through MinDist on clouds whose keep pattern is built in,
RandomSampling and MaxDensity against the numpy filters with the same draw, the densities against
the oracle's, and the normals a sampled reference carries.
"""
import numpy as np
import pytest

import chain_reference as cr
from aicp_mapping_amd import synthetic as sy

f32 = np.float32
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def run_case(ctx, L, case):
    lists = [(), ()]
    lists[case["side"]] = case["filters"]
    ch = cr.make_chain(L, lists[0], lists[1], seed=case["seed"])
    return ctx.chain_filter(ch, case["side"], case["pts"], densities=cr.has_densities(case))


@gpu
@pytest.mark.parametrize("name", sorted(cr.cases()))
def test_case_matches_the_reference(ctx, L, oracle, name):
    """Kept indices exact and ascending, the count after each filter; where the pattern is built
    into the cloud (compaction edges, points on the radius, |coord| == minDist), against it too."""
    case = cr.cases()[name]
    got = run_case(ctx, L, case)
    cr.compare(case, got)
    assert got["n"] == len(got["index"]) == (got["counts"][-1] if got["counts"] else len(case["pts"]))


@gpu
def test_random_sampling_draws_by_the_position_after_min_dist(ctx, L):
    """MinDist -> RandomSampling in one list equals the two filters run as two calls and composed:
    the second call's cloud is what MinDist left, so its indices are the draw's (a MinDist that
    keeps everything holds position 0 there, so that RandomSampling keeps its slot)."""
    case = cr.cases()["mindist_random"]
    both = run_case(ctx, L, case)
    first = ctx.chain_filter(cr.make_chain(L, [case["filters"][0]], (), seed=case["seed"]), cr.REFERENCE, case["pts"])
    keep_all = dict(kind=cr.MIN_DIST, dim=0, min_dist=-1.0)
    second = ctx.chain_filter(cr.make_chain(L, [keep_all, case["filters"][1]], (), seed=case["seed"]), cr.REFERENCE,
                              case["pts"][first["index"]])
    assert second["counts"][0] == first["n"]
    assert np.array_equal(first["index"][second["index"]], both["index"])
    assert 0 < both["n"] < first["n"] < len(case["pts"])


def _ulps(a, b):
    """Units in the last place between positive float32 arrays (+inf against +inf: 0)."""
    ia = np.asarray(a, f32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def scene_cloud():
    return np.ascontiguousarray(sy.make_pair(3000, 3000, seed=7, half=12.0).read, f32)


def _densities(ctx, L, pts, knn):
    ch = cr.make_chain(L, (), [dict(kind=cr.SN, knn=knn, keep_densities=1)])
    got = ctx.chain_filter(ch, cr.READING, pts, densities=True)
    assert got["n"] == len(pts) and got["counts"] == [len(pts)] and np.array_equal(got["index"], np.arange(len(pts)))
    return got["densities"]


@gpu
@pytest.mark.parametrize("knn", [10, 20, 30])
def test_densities_match_the_oracle(ctx, L, oracle, knn):
    """Derived bound: 4 float ulp (the volume comes from a double cube that may differ from std::pow
    by 2 double ulp, at most 1 float ulp after the cast; the division adds one more; the margin is
    twice that). Measured on the MI355X: 0 ulp at K = 10, 20 and 30, no density of the 3 000
    differs (profiles/chain_gpu_tests.log), so the test asks for equality. (With the native square
    root, __fsqrt_rn, for the radius it measured 7 ulp: the radius is cubed.)"""
    pts = scene_cloud()
    dev = _densities(ctx, L, pts, knn)
    want = oracle.surface_normals(pts, knn)[1]
    d = _ulps(dev, want)
    print(f"knn {knn}: densities differ from the oracle's by at most {int(d.max())} ulp ({int(np.sum(d > 0))} of {len(d)} differ)")
    assert d.max() == 0


@gpu
def test_density_of_a_duplicated_point_is_infinite(ctx, L, oracle):
    rng = np.random.default_rng(5)
    pts = rng.uniform(-2, 2, (500, 3)).astype(f32)
    # an exact 10-fold duplicate whose float mean is the point itself (10 x and 10 x / 10 are exact
    # for coordinates of a few bits): radius 0, density +inf. (A duplicate of arbitrary floats has a
    # mean one rounding away, and a huge finite density.)
    pts[100:110] = (0.5, -1.25, 1.0)
    want = oracle.surface_normals(pts, 10)[1]
    assert np.all(np.isposinf(want[100:110]))
    dev = _densities(ctx, L, pts, 10)
    assert np.all(np.isposinf(dev[100:110])) and np.all(np.isposinf(want[100:110]))
    assert np.array_equal(np.isinf(dev), np.isinf(want)) and _ulps(dev, want).max() <= 4


@gpu
def test_densities_of_a_cloud_of_fewer_points_than_knn(ctx, L, oracle):
    dev = _densities(ctx, L, cr.CUBE8, 10)
    want = oracle.surface_normals(cr.CUBE8, 10)[1]
    assert np.array_equal(dev, want) and np.all(dev == f32(cr.CUBE8_DENSITY))
    pts = np.random.default_rng(6).uniform(-1, 1, (7, 3)).astype(f32)
    assert _ulps(_densities(ctx, L, pts, 20), oracle.surface_normals(pts, 20)[1]).max() <= 4


@gpu
def test_max_density_on_a_scene_cloud_at_its_median_density(ctx, L):
    """The reference takes the device's densities (checked above on their own) and the draw."""
    pts = scene_cloud()
    dens = _densities(ctx, L, pts, 10)
    md = float(np.median(dens))
    case = dict(pts=pts, side=cr.READING, seed=17,
                filters=[dict(kind=cr.SN, knn=10, keep_densities=1), dict(kind=cr.MAX_DENSITY, max_density=md)])
    got = run_case(ctx, L, case)
    assert np.array_equal(got["densities"], dens)
    cr.compare(case, got)
    below = int(np.sum(dens <= f32(md)))
    print(f"maxDensity {md}: {got['n']} of {len(pts)} kept, {below} without a draw")
    assert below < got["n"] < len(pts) and got["counts"] == [len(pts), got["n"]]


@gpu
def test_sampled_reference_carries_the_full_clouds_normals(ctx, L):
    pts = scene_cloud()
    ch = cr.make_chain(L, [dict(kind=cr.SN, knn=10), dict(kind=cr.RANDOM, prob=0.5)], (), seed=9)
    got = ctx.chain_filter(ch, cr.REFERENCE, pts, normals=True)
    full, _ = ctx.normals(pts, 10)
    assert 1000 < got["n"] < 2000
    assert got["normals"].tobytes() == full[got["index"]].tobytes()


@gpu
def test_surface_normal_behind_a_dropping_filter(ctx, L, oracle):
    """MinDist -> SurfaceNormal -> ...: the one order in which the host reads a count before the last
    filter (it sizes the SurfaceNormal's tree). Densities and normals are those of the cloud MinDist
    leaves; test_case_matches_the_reference[mindist_density] holds the kept list."""
    case = cr.cases()["mindist_density"]
    pts = case["pts"]
    kept = np.nonzero(cr.min_dist_keep(pts, -1, 2.0))[0]
    got = run_case(ctx, L, case)
    assert got["counts"][:2] == [len(kept), len(kept)] and 0 < got["n"] < len(kept) < len(pts)
    assert np.array_equal(got["densities"], oracle.surface_normals(pts[kept], 10)[1])
    ch = cr.make_chain(L, [case["filters"][0], dict(kind=cr.SN, knn=10), dict(kind=cr.RANDOM, prob=0.5)], (), seed=21)
    g = ctx.chain_filter(ch, cr.REFERENCE, pts, normals=True)
    full, _ = ctx.normals(pts[kept], 10)
    assert 0 < g["n"] < len(kept) and np.all(np.isin(g["index"], kept))
    assert g["normals"].tobytes() == full[np.searchsorted(kept, g["index"])].tobytes()


@gpu
def test_chain_filter_refuses_what_it_cannot_run(ctx, L):
    pts = scene_cloud()[:100]
    bad = cr.make_chain(L, (), [dict(kind=cr.MAX_DENSITY, max_density=5.0)])
    with pytest.raises(L.AicpError) as e:
        ctx.chain_filter(bad, cr.READING, pts)
    assert e.value.code == L.AICP_ERR_INVALID
    odd = cr.make_chain(L, (), [dict(kind=cr.SN, knn=7, keep_densities=1), dict(kind=cr.MAX_DENSITY, max_density=5.0)])
    with pytest.raises(L.AicpError) as e:
        ctx.chain_filter(odd, cr.READING, pts)
    assert e.value.code == L.AICP_ERR_UNSUPPORTED
    for lim in (float("inf"), float("nan"), -1.0):   # an infinite limit would keep unmatched readings
        T, st, cs, rc = ctx.register_chain(pts, pts, L.default_config(), cr.make_chain(L, (), (), max_dist_d2=lim),
                                           raise_on_error=False)
        assert rc == L.AICP_ERR_INVALID, lim
