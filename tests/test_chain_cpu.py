"""The sampled chains on the CPU: the chain parser on the reference's chain files
(tests/golden/chains), the draw against its numpy restatement bit for bit and statistically, and the
numpy reference's own tests: every mutation of chain_reference.MUTATIONS is caught by at least one
of the cases the GPU tests run, with simulate() standing in for the device.
"""
import math
import os

import numpy as np
import pytest

import chain_reference as cr

f32 = np.float32
CHAINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chains")
SERVED = ("Besl92_pt2point", "icp_3D_cfg_max", "icp_3D_cfg_trimmed", "icp_3Dtesting_cfg", "icp_3Dtesting_cfg2",
          "icp_max_atlas_finals", "icp_trimmed_atlas_finals")
REFUSED = ("Chen91_pt2plane", "icp_tutorial_cfg")
PLAIN = (os.path.join(CHAINS, "icp_autotuned.yaml"), os.path.join(CHAINS, "icp_2Dtesting_cfg.yaml"),
         os.path.join(CHAINS, "..", "icp_autotuned_default.yaml"))


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


def _path(name):
    return os.path.join(CHAINS, name + ".yaml")


# ------------------------------------------------------------------ the parser -------------
def _sn(L, knn, dens):
    return dict(kind=L.AICP_FILTER_SURFACE_NORMAL, knn=knn, keep_densities=dens)


def _cfg_values(c):
    return (c.knn_normals, c.nn_epsilon, c.trimmed_ratio, c.max_iter, c.min_diff_rot, c.min_diff_trans, c.smooth_length,
            c.bucket_size, c.knn_match)


def _expected(L):
    """What each of the seven files holds, written out: (reference list, reading list, outlier rule,
    limit, aicp_icp_config values)."""
    md = dict(kind=L.AICP_FILTER_MIN_DIST, dim=-1, min_dist=1.0)
    rs05, rs5 = dict(kind=L.AICP_FILTER_RANDOM_SAMPLING, prob=f32(0.05)), dict(kind=L.AICP_FILTER_RANDOM_SAMPLING, prob=0.5)
    mx = dict(kind=L.AICP_FILTER_MAX_DENSITY, max_density=50.0)
    read3d = [_sn(L, 10, 1), mx]
    ref3d = [_sn(L, 10, 0), rs5]
    tr, mxd = L.AICP_OUTLIER_TRIMMED_DIST, L.AICP_OUTLIER_MAX_DIST
    plane100 = (10, 0.0, f32(0.75), 100, f32(0.001), f32(0.001), 4, 8, 1)
    # (the MaxDist files name no ratio: trimmed_ratio keeps libpointmatcher's default, 0.85, unused)
    plane100_max = (10, 0.0, f32(0.85), 100, f32(0.001), f32(0.001), 4, 8, 1)
    return {
        "Besl92_pt2point": ([md, rs05], [md, rs05], tr, 0.0, (0, f32(3.16), f32(0.75), 150, f32(0.001), f32(0.01), 4, 8, 1)),
        "icp_3D_cfg_max": (ref3d, read3d, mxd, f32(0.05), plane100_max),
        "icp_max_atlas_finals": (ref3d, read3d, mxd, f32(0.05), plane100_max),
        "icp_3D_cfg_trimmed": (ref3d, read3d, tr, 0.0, plane100),
        "icp_3Dtesting_cfg2": (ref3d, read3d, tr, 0.0, plane100),
        "icp_trimmed_atlas_finals": (ref3d, read3d, tr, 0.0, plane100),
        "icp_3Dtesting_cfg": ([_sn(L, 10, 0)], read3d, tr, 0.0, (10, 0.0, f32(0.75), 40, f32(0.001), f32(0.01), 4, 8, 1)),
    }


@pytest.mark.parametrize("name", SERVED)
def test_served_files_parse_to_their_lists(L, name):
    ref, read, outlier, limit, cfg = _expected(L)[name]
    rc, c, ch = L.parse_pm_chain(_path(name))
    assert rc == L.AICP_OK
    assert ch.side(L.AICP_CHAIN_REFERENCE) == ref
    assert ch.side(L.AICP_CHAIN_READING) == read
    assert (ch.outlier, ch.outlier_limit_d2, ch.seed) == (outlier, limit, 0)
    assert _cfg_values(c) == cfg and c.nn_max_dist == f32(np.inf)
    # unused filter slots stay zero
    for side in (0, 1):
        for q in range(ch.n_filters[side], L.AICP_CHAIN_MAX_FILTERS):
            assert bytes(ch.filters[side][q]) == bytes(32)


@pytest.mark.parametrize("name", REFUSED)
def test_sampling_surface_normal_files_stay_refused(L, name):
    assert L.parse_pm_chain(_path(name))[0] == L.AICP_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", SERVED + REFUSED)
def test_parse_pm_yaml_still_refuses_all_nine(L, name):
    assert L.parse_pm_yaml(_path(name))[0] == L.AICP_ERR_UNSUPPORTED


@pytest.mark.parametrize("path", PLAIN)
def test_accepted_files_give_the_same_config_through_both_parsers(L, path):
    rc0, c0 = L.parse_pm_yaml(path)
    rc1, c1, ch = L.parse_pm_chain(path)
    assert rc0 == rc1 == L.AICP_OK
    assert bytes(c0) == bytes(c1)
    assert (ch.outlier, ch.seed) == (L.AICP_OUTLIER_TRIMMED_DIST, 0)
    for side in (0, 1):
        assert all(f["kind"] == L.AICP_FILTER_SURFACE_NORMAL for f in ch.side(side))


def test_an_all_zero_chain_is_no_filters_trimmed_dist(L):
    ch = L.Chain()
    assert bytes(ch) == bytes(len(bytes(ch)))
    assert ch.n_filters[0] == ch.n_filters[1] == 0 and ch.outlier == L.AICP_OUTLIER_TRIMMED_DIST


def _text(read="", ref="  - SurfaceNormalDataPointsFilter:\n      knn: 10\n", minimizer="PointToPlaneErrorMinimizer",
          outlier="  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"):
    return ((f"readingDataPointsFilters:\n{read}\n" if read else "") + (f"referenceDataPointsFilters:\n{ref}\n" if ref else "")
            + "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n\n" + f"outlierFilters:\n{outlier}\n"
            + f"errorMinimizer:\n  {minimizer}\n\n"
            + "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n\n"
            + "inspector:\n  NullInspector\n\nlogger:\n  FileLogger\n")


SN_D = "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      keepDensities: 1\n"
SN_0 = "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
MAXD = "  - MaxDensityDataPointsFilter:\n      maxDensity: 50\n"
RAND = "  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
MIND = "  - MinDistDataPointsFilter:\n      minDist: 1.0\n"
INVALID = {
    "max_density_without_surface_normal": _text(read=MAXD),
    "max_density_without_keep_densities": _text(read=SN_0 + MAXD),
    "max_density_before_its_surface_normal": _text(read=MAXD + SN_D),
    "prob_above_one": _text(read="  - RandomSamplingDataPointsFilter:\n      prob: 1.5\n"),
    "prob_negative": _text(read="  - RandomSamplingDataPointsFilter:\n      prob: -0.1\n"),
    "max_density_zero": _text(read=SN_D + "  - MaxDensityDataPointsFilter:\n      maxDensity: 0\n"),
    "dim_three": _text(read="  - MinDistDataPointsFilter:\n      dim: 3\n      minDist: 1.0\n"),
    "dim_minus_two": _text(read="  - MinDistDataPointsFilter:\n      dim: -2\n"),
    "max_dist_negative": _text(outlier="  - MaxDistOutlierFilter:\n      maxDist: -0.5\n"),
    "max_dist_infinite": _text(outlier="  - MaxDistOutlierFilter:\n      maxDist: inf\n"),
    "max_dist_nan": _text(outlier="  - MaxDistOutlierFilter:\n      maxDist: nan\n"),
}
UNSUPPORTED = {
    "five_filters": _text(read=MIND + RAND + MIND + RAND + MIND),
    "two_surface_normals": _text(read=SN_D + RAND + SN_D),
    "knn_of_used_normals": _text(ref="  - SurfaceNormalDataPointsFilter:\n      knn: 15\n" + RAND),
    "knn_of_used_densities": _text(read="  - SurfaceNormalDataPointsFilter:\n      knn: 5\n      keepDensities: 1\n" + MAXD),
    "sampling_surface_normal": _text(read="  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"),
    "bounding_box": _text(read="  - BoundingBoxDataPointsFilter:\n      xMin: -1\n"),
    "max_dist_data_points_filter": _text(read="  - MaxDistDataPointsFilter:\n      maxDist: 10\n"),
    "two_outlier_filters": _text(outlier="  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n  - MaxDistOutlierFilter:\n"
                                         "      maxDist: 1\n"),
    "median_dist_outlier": _text(outlier="  - MedianDistOutlierFilter:\n      factor: 3\n"),
    "plane_without_reference_normals": _text(read=RAND, ref=RAND),
    "plane_without_reference_list": _text(read=RAND, ref=""),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_chain_texts(L, tmp_path, name):
    p = tmp_path / "c.yaml"
    p.write_text(INVALID[name])
    assert L.parse_pm_chain(str(p))[0] == L.AICP_ERR_INVALID


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_unsupported_chain_texts(L, tmp_path, name):
    p = tmp_path / "c.yaml"
    p.write_text(UNSUPPORTED[name])
    assert L.parse_pm_chain(str(p))[0] == L.AICP_ERR_UNSUPPORTED


def test_unused_surface_normal_may_have_any_knn(L, tmp_path):
    """A reading's SurfaceNormal whose densities nobody consumes, a point-to-point reference's: not run."""
    p = tmp_path / "c.yaml"
    p.write_text(_text(read="  - SurfaceNormalDataPointsFilter:\n      knn: 7\n" + RAND,
                       ref="  - SurfaceNormalDataPointsFilter:\n      knn: 7\n" + RAND, minimizer="PointToPointErrorMinimizer"))
    rc, c, ch = L.parse_pm_chain(str(p))
    assert rc == L.AICP_OK and c.knn_normals == 0 and ch.n_filters[0] == ch.n_filters[1] == 2


def test_max_dist_limit_is_the_parameter_as_written(L, tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text(_text(outlier="  - MaxDistOutlierFilter:\n      maxDist: 0.3\n"))
    rc, c, ch = L.parse_pm_chain(str(p))
    assert rc == L.AICP_OK and ch.outlier == L.AICP_OUTLIER_MAX_DIST and ch.outlier_limit_d2 == f32(0.3)


# ------------------------------------------------------------------ the draw ---------------
def _lib_uniform(L, seed, slot, idx):
    return np.array([L.lib.aicp_hip_chain_uniform(seed, slot, int(i)) for i in idx], f32)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_draw_equals_its_restatement_bit_for_bit(L, seed):
    idx = np.arange(2 ** 16)
    edge = np.array([2 ** 32 - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1])
    i = np.r_[idx, edge]
    for slot in range(8):
        assert _lib_uniform(L, seed, slot, i).tobytes() == cr.uniform(seed, slot, i).tobytes(), slot


N_DRAWS = 2 ** 20


@pytest.mark.parametrize("seed", [0, 1])
def test_draw_statistics(L, seed):
    """Bounds derived from the uniform law, 5 standard deviations each: a sound mixer passes with
    probability about 1 - 1e-5. The 2^20 draws are the library's own (aicp_hip_chain_uniform, one
    call each), and equal the restatement's over the whole range; the second slot's are the
    restatement's (held bit for bit above)."""
    fn = L.lib.aicp_hip_chain_uniform
    r = np.fromiter((fn(seed, 1, i) for i in range(N_DRAWS)), f32, N_DRAWS)
    assert r.tobytes() == cr.uniform(seed, 1, np.arange(N_DRAWS)).tobytes()
    assert r.dtype == f32 and r.min() >= 0 and r.max() < 1
    k = r.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.rint(k))
    assert abs(r.astype(np.float64).mean() - 0.5) <= 5 / math.sqrt(12 * N_DRAWS)
    for p in (0.05, 0.5):
        assert abs(np.mean(r < f32(p)) - p) <= 5 * math.sqrt(p * (1 - p) / N_DRAWS), p
    other = cr.uniform(seed, 5, np.arange(N_DRAWS))
    agree = np.mean((r < f32(0.5)) == (other < f32(0.5)))
    assert abs(agree - 0.5) <= 5 * math.sqrt(0.25 / N_DRAWS)


# ------------------------------------------------------------------ the reference's own tests
def test_reference_agrees_with_itself_on_every_case(oracle):
    for name, case in cr.cases().items():
        cr.compare(case, cr.simulate(case))


@pytest.mark.parametrize("mut", cr.MUTATIONS)
def test_every_mutation_is_caught_by_a_gpu_case(oracle, mut):
    caught = []
    for name, case in cr.cases().items():
        try:
            cr.compare(case, cr.simulate(case, mut))
        except cr.Mismatch:
            caught.append(name)
    print(mut, "caught by", len(caught), "cases:", caught[:6])
    assert caught, mut


def test_the_cube_is_saturated_everywhere(oracle):
    """Every point of the 8-point cube has the same density (all 8 points are every point's
    neighbours, mean 0, radius sqrt(3)/2 exactly), so MaxDensity sees nbSaturated == nbPointsIn."""
    dens = oracle.surface_normals(cr.CUBE8, 10)[1]
    assert np.all(dens == dens[0]) and dens[0] == f32(cr.CUBE8_DENSITY)


def test_the_lone_case_tells_integer_from_float_division(oracle):
    case = cr.lone_case()
    keep_int = cr.run_filters(case["pts"], case["filters"], case["side"], case["seed"])["index"]
    keep_flt = cr.run_filters(case["pts"], case["filters"], case["side"], case["seed"], mut="float_saturation")["index"]
    assert case["top"] in keep_int and case["top"] not in keep_flt
