"""Raw readings in the two map localization streams, the CPU side: the C ABI and its Python
bindings are there, and the host restatement of tests/raw_stream_reference.py has the properties
the GPU tests (tests/test_raw_stream.py) rely on. Its fixtures are pinned here: the drop / merge /
re-filter pattern, and that App's order and the swapped one keep different points in debug mode."""
import os
import re

import numpy as np
import pytest

import built_map_reference as bm
import localization_reference as lr
import raw_stream_reference as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aicp_hip_map_sequence_run_raw", "aicp_hip_built_map_sequence_run_raw", "aicp_hip_test_ingest")


@pytest.fixture(scope="module")
def prior(oracle):
    return rs.prior_world(oracle)


@pytest.fixture(scope="module")
def built(oracle):
    return rs.built_world(oracle)


def test_header_declares_and_python_binds_the_new_symbols():
    import aicp_mapping_amd._lib as L

    txt = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes, name
    # out_kept and the readings' pre-filter are part of the two stream calls
    assert len(L.lib.aicp_hip_map_sequence_run_raw.argtypes) == len(L.lib.aicp_hip_map_sequence_run.argtypes) + 2
    assert (len(L.lib.aicp_hip_built_map_sequence_run_raw.argtypes) ==
            len(L.lib.aicp_hip_built_map_sequence_run.argtypes) + 2)


def same_records(a, b, keys):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert x[k] == y[k], (i, k, x[k], y[k])
        np.testing.assert_array_equal(x["T"], y["T"])
        assert (x["stats"].iterations, x["stats"].nn_points_touched) == (y["stats"].iterations,
                                                                        y["stats"].nn_points_touched), i
        if x["accepted"]:
            np.testing.assert_array_equal(x["corrected_origin"], y["corrected_origin"])


def test_prior_map_robot_mode_is_the_replay_of_the_prefiltered_readings(oracle, prior):
    mp, raws, poses, origins = prior
    rec, final = rs.replay_prior_raw(oracle, mp, raws, poses, origins, **lr.PARAMS)
    kept = [oracle.prefilter(r)["out"] for r in raws]
    exp, efinal = lr.replay(oracle, mp, kept, poses, origins, **lr.PARAMS)
    same_records(rec, exp, ("status", "accepted", "merged", "refiltered", "map_points", "crop_points"))
    np.testing.assert_array_equal(final, efinal)
    assert [r["kept"] for r in rec] == [len(k) for k in kept]
    # the fixture: every reading registers, two drops, merges at 0 and 4, re-filters at 0 and 6
    assert [r["status"] for r in rec] == [0] * 8
    assert [r["accepted"] for r in rec] == [1, 1, 0, 1, 1, 0, 1, 1]
    assert [i for i, r in enumerate(rec) if r["merged"]] == [0, 4]
    assert [i for i, r in enumerate(rec) if r["refiltered"]] == [0, 6]
    assert all(5120 <= r["kept"] <= 5204 for r in rec), [r["kept"] for r in rec]
    assert all(len(r) == rs.N_RAW for r in raws)


def test_built_map_robot_mode_is_the_replay_of_the_prefiltered_readings(oracle, built):
    first, raws, poses, origins = built
    rec, final = rs.replay_built_raw(oracle, first, raws, poses, origins, **bm.PARAMS)
    kept = [oracle.prefilter(r)["out"] for r in raws]
    exp, efinal = bm.replay(oracle, first, kept, poses, origins, **bm.PARAMS)
    same_records(rec, exp, ("status", "accepted", "is_reference", "map_points", "crop_points", "overlap", "counts",
                            "ratio"))
    np.testing.assert_array_equal(final, efinal)
    assert [r["kept"] for r in rec] == [len(k) for k in kept]


def test_prior_map_debug_mode_orders_differ(oracle, prior):
    mp, raws, poses, origins = prior
    app, _ = rs.replay_prior_raw(oracle, mp, raws, poses, origins, debug=True, **lr.PARAMS)
    swp, sfinal = rs.replay_prior_raw(oracle, mp, raws, poses, origins, debug=True, order="swapped", **lr.PARAMS)
    for rec in (app, swp):
        assert [r["status"] for r in rec] == [0] * 8
        assert [r["accepted"] for r in rec] == [1, 1, 0, 1, 1, 0, 1, 1]
        assert [i for i, r in enumerate(rec) if r["merged"]] == [0, 4]
        assert [i for i, r in enumerate(rec) if r["refiltered"]] == [0, 6]
    ka, ks = [r["kept"] for r in app], [r["kept"] for r in swp]
    assert ka[0] == ks[0]  # initialT_ is still the identity
    assert all(a != s for a, s in zip(ka[1:], ks[1:])), (ka, ks)
    assert (ka[1], ks[1]) == (5226, 5151)
    # the swapped order is what the pre-filtered stream's debug flag does to readings filtered beforehand
    kept = [oracle.prefilter(r)["out"] for r in raws]
    exp, efinal = lr.replay(oracle, mp, kept, poses, origins, debug=True, **lr.PARAMS)
    same_records(swp, exp, ("status", "accepted", "merged", "refiltered", "map_points", "crop_points"))
    np.testing.assert_array_equal(sfinal, efinal)


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_built_map_fixture_drops_and_appends(oracle, built, debug):
    first, raws, poses, origins = built
    rec, final = rs.replay_built_raw(oracle, first, raws, poses, origins, debug=debug, **bm.PARAMS)
    assert [r["status"] for r in rec] == [0] * rs.N_BUILT
    assert [r["accepted"] for r in rec].count(0) >= 1
    assert [r["accepted"] for r in rec] == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    assert [i for i, r in enumerate(rec) if r["is_reference"]] == [2, 6, 9]
    assert len(final) == len(first) + sum(r["kept"] for r in rec if r["is_reference"])
    if debug:  # and the orders differ here too
        swp, _ = rs.replay_built_raw(oracle, first, raws, poses, origins, debug=True, order="swapped", **bm.PARAMS)
        assert [r["kept"] for r in rec][1:] != [r["kept"] for r in swp][1:]


def test_built_map_reference_jumps_drop_nothing_at_this_size(oracle, built):
    first = built[0]
    raws, poses, origins = rs._stream(rs.N_BUILT, bm.JUMPS)
    rec, _ = rs.replay_built_raw(oracle, first, raws, poses, origins, **bm.PARAMS)
    assert [r["status"] for r in rec] == [0] * rs.N_BUILT and all(r["accepted"] for r in rec)
    assert [i for i, r in enumerate(rec) if r["is_reference"]] == [2, 5, 8]


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_an_emptied_reading_is_invalid_at_its_index(oracle, prior, built, debug):
    assert len(oracle.prefilter(rs.scattered())["out"]) == 0
    mp, raws, poses, origins = prior
    bad = raws[:3] + [rs.scattered()] + raws[4:]
    rec, final = rs.replay_prior_raw(oracle, mp, bad, poses, origins, debug=debug, **lr.PARAMS)
    assert [r["status"] for r in rec] == [0, 0, 0, rs.AICP_ERR_INVALID]
    assert rec[3]["kept"] == 0 and not rec[3]["accepted"]
    good, gfinal = rs.replay_prior_raw(oracle, mp, raws[:3], poses[:3], origins[:3], debug=debug, **lr.PARAMS)
    np.testing.assert_array_equal(final, gfinal)  # the map is as after reading 2
    first, raws, poses, origins = built
    bad = raws[:3] + [rs.scattered()] + raws[4:]
    rec, final = rs.replay_built_raw(oracle, first, bad, poses, origins, debug=debug, **bm.PARAMS)
    assert [r["status"] for r in rec] == [0, 0, 0, rs.AICP_ERR_INVALID] and rec[3]["kept"] == 0
    assert rec[2]["is_reference"] and len(final) == len(first) + rec[2]["kept"]
