"""App's localization stream on the device-resident prior map (aicp_hip_map_sequence_run,
PriorMap.sequence_run) against the host restatement of tests/localization_reference.py (the
oracle's crop, ICP, transform, corrected origin, Matrix4f product and pre-filter) and against the
hand composition of the existing entry points (register_batch, merge, prefilter), window by
window. Fixture and expected patterns: tests/test_localization_cpu.py pins them on the CPU."""
import numpy as np
import pytest

import localization_reference as lr
from aicp_mapping_amd import synthetic as sy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(oracle):
    mp = lr.make_map(oracle)
    reads, poses, origins = lr.make_stream(10, lr.JUMPS)
    return mp, reads, poses, origins


def params(L, **kw):
    return L.default_localization_params(**dict(lr.PARAMS, **kw))


def run(ctx, mp, reads, poses, prm, cfg=None, raise_on_error=True):
    from aicp_mapping_amd.prior_map import PriorMap

    pm = PriorMap(ctx, mp)
    T, res, done, rc = pm.sequence_run(reads, poses, cfg=cfg, params=prm, raise_on_error=raise_on_error)
    final = pm.getCloud()
    pm.free()
    return T, res, done, rc, final


def check_against_replay(oracle, mp, reads, poses, origins, debug, T, res, final, cfg=None):
    """The free-running replay takes the same decisions; the forced replay (state from the
    device's corrections) sees the same maps and crops, registers in the same iterations with the
    same NN touch counts, and ends with the same map, bit for bit."""
    n = len(res)
    free, _ = lr.replay(oracle, mp, reads[:n], poses[:n], origins[:n], cfg=cfg, debug=debug, **lr.PARAMS)
    for k in ("status", "accepted", "merged", "refiltered"):
        assert [r[k] for r in res] == [r[k] for r in free], k
    forced, fmap = lr.replay(oracle, mp, reads[:n], poses[:n], origins[:n], cfg=cfg, debug=debug, forced_T=T,
                             **lr.PARAMS)
    for i, (d, r) in enumerate(zip(res, forced)):
        for k in ("status", "accepted", "merged", "refiltered", "map_points", "crop_points"):
            assert d[k] == r[k], (i, k, d[k], r[k])
        if r["status"]:
            continue
        assert d["icp"]["iterations"] == r["stats"].iterations, i
        assert (d["icp"]["nn_points_touched"], d["icp"]["nn_nodes_touched"]) == (r["stats"].nn_points_touched,
                                                                               r["stats"].nn_nodes_touched), i
        assert d["icp"]["trimmed_ratio"] == np.float32(0.5)
        rr, tt = sy.rot_err(r["T"], T[i])
        assert rr < 1e-6 and tt < 1e-5, (i, rr, tt)
        if r["accepted"]:
            np.testing.assert_allclose(d["corrected_origin"], r["corrected_origin"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(final, fmap)
    return free


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_stream_equals_replay(ctx, oracle, L, world, debug):
    mp, reads, poses, origins = world
    T, res, done, rc, final = run(ctx, mp, reads, poses, params(L, debug=debug))
    assert rc == 0 and done == 10
    tm = ctx.last_localization_timing()
    check_against_replay(oracle, mp, reads, poses, origins, debug, T, res, final)
    assert [r["accepted"] for r in res] == [1, 1, 0, 1, 1, 0, 1, 1, 1, 1]
    assert [i for i, r in enumerate(res) if r["merged"]] == [0, 4, 8]
    assert [i for i, r in enumerate(res) if r["refiltered"]] == [0, 6]
    # windows of 1, 3, 1, 1, 1, 2, 1 readings in robot mode, one reading each in debug mode
    assert (tm["windows"], tm["merges"], tm["refilters"]) == (10 if debug else 7, 3, 2)
    assert tm["wall_ms"] >= tm["device_ms"] > 0


@pytest.mark.parametrize("debug,accepted", [(False, [1, 1, 1]), (True, [1, 0, 0])], ids=["robot", "debug"])
def test_first_reading_is_never_dropped(ctx, oracle, L, world, debug, accepted):
    mp = world[0]
    reads, poses, origins = lr.make_stream(3, lr.JUMP_ON_0)
    T, res, done, rc, final = run(ctx, mp, reads, poses, params(L, debug=debug))
    assert rc == 0 and done == 3
    assert abs(T[0][1, 3]) > 0.4  # beyond max_correction_magnitude, and still accepted
    assert (res[0]["accepted"], res[0]["merged"], res[0]["refiltered"]) == (1, 1, 1)
    assert [r["accepted"] for r in res] == accepted
    check_against_replay(oracle, mp, reads, poses, origins, debug, T, res, final)


def compose(ctx, L, mp, reads, poses, prm, cfg=None):
    """The stream from the existing entry points, one window at a time: register_batch, then the
    merges and re-filters App's counters ask for (host bookkeeping, every merged reading uploaded a
    second time)."""
    from aicp_mapping_amd.prior_map import PriorMap

    pm = PriorMap(ctx, mp)
    n, p, n_clouds = len(reads), 0, 0
    Ts, stats, flags = [], [], []
    mc = np.float32(prm.max_correction_magnitude)
    merge = bool(prm.flags & L.AICP_LOC_MERGE)
    while p < n:
        w = L.localization_window(n_clouds, prm, n - p)
        T, st, rc = pm.register_batch(reads[p:p + w], poses[p:p + w], prm.crop_min, prm.crop_max, cfg=cfg)
        assert rc == 0
        for i in range(w):
            Ts.append(T[i])
            stats.append(st[i])
            f = dict(accepted=0, merged=0, refiltered=0)
            flags.append(f)
            if n_clouds != 0 and any(abs(T[i][k, 3]) > mc for k in range(3)):
                continue
            n_clouds += 1
            f["accepted"] = 1
            if merge and (n_clouds - 1) % prm.reference_update_frequency == 0:
                pm.merge(reads[p + i], T[i])
                f["merged"] = 1
            if merge and prm.map_refilter_every > 0 and (n_clouds - 1) % prm.map_refilter_every == 0:
                pm.prefilter()
                f["refiltered"] = 1
        p += w
    final = pm.getCloud()
    pm.free()
    return np.stack(Ts), stats, flags, final


def test_robot_mode_equals_hand_composition(ctx, L, world):
    mp, reads, poses, origins = world
    prm = params(L)
    T, res, done, rc, final = run(ctx, mp, reads, poses, prm)
    assert rc == 0 and done == 10
    Tc, stc, fc, finalc = compose(ctx, L, mp, reads, poses, prm)
    np.testing.assert_array_equal(T, Tc)
    for i in range(10):
        assert res[i]["icp"] == stc[i], i
        assert {k: res[i][k] for k in ("accepted", "merged", "refiltered")} == fc[i], i
    np.testing.assert_array_equal(final, finalc)
    T2, res2, done2, rc2, final2 = run(ctx, mp, reads, poses, prm)  # repeatable
    np.testing.assert_array_equal(T, T2)
    assert res == res2 and done2 == 10
    np.testing.assert_array_equal(final, final2)


def test_merge_off_is_one_batch(ctx, L, world):
    from aicp_mapping_amd.prior_map import PriorMap

    mp, reads, poses, origins = world
    T, res, done, rc, final = run(ctx, mp, reads, poses, params(L, merge=False))
    assert rc == 0 and done == 10 and ctx.last_localization_timing()["windows"] == 1
    np.testing.assert_array_equal(final, mp)
    assert not any(r["merged"] or r["refiltered"] for r in res)
    pm = PriorMap(ctx, mp)
    Tb, stb, rcb = pm.register_batch(reads, poses, lr.PARAMS["crop_min"], lr.PARAMS["crop_max"])
    pm.free()
    assert rcb == 0
    np.testing.assert_array_equal(T, Tb)
    assert [r["icp"] for r in res] == stb
    mc = np.float32(lr.PARAMS["max_correction_magnitude"])  # the drop test still runs (no count without it)
    exp = [int(i == 0 or not any(abs(Tb[i][k, 3]) > mc for k in range(3))) for i in range(10)]
    assert [r["accepted"] for r in res] == exp and exp[2] == exp[5] == 0
    assert all(r["map_points"] == len(mp) for r in res)


def test_stream_ends_at_the_failing_reading(ctx, oracle, L, world):
    mp, reads, poses, origins = world
    prm = params(L)
    # reading 2 sits inside the window of readings 1..3: reading 1 is committed, reading 3 is not
    far = np.array(poses[2], np.float64)
    far[:3, 3] += (200.0, 0.0, 0.0)
    poses_far = poses[:2] + [far] + poses[3:]
    T, res, done, rc, final = run(ctx, mp, reads, poses_far, prm, raise_on_error=False)
    assert rc == L.AICP_ERR_INVALID and done == 3 and len(res) == 3
    assert [r["status"] for r in res] == [0, 0, L.AICP_ERR_INVALID] and res[2]["crop_points"] == 0
    # the replay ends there too, and the map holds exactly the merge and re-filter of reading 0
    check_against_replay(oracle, mp, reads, poses_far, origins, False, T, res, final)
    assert [(r["merged"], r["refiltered"]) for r in res] == [(1, 1), (0, 0), (0, 0)]
    with pytest.raises(L.AicpError) as e:
        run(ctx, mp, reads, poses_far, prm)
    assert e.value.code == L.AICP_ERR_INVALID

    cfg = L.default_config(nn_max_dist=5.0)
    shifted = (reads[2] + np.float32([200.0, 0.0, 0.0])).astype(np.float32)
    reads_bad = reads[:2] + [shifted] + reads[3:]
    T, res, done, rc, final = run(ctx, mp, reads_bad, poses, prm, cfg=cfg, raise_on_error=False)
    assert rc == L.AICP_ERR_CONVERGENCE and done == 3 and len(res) == 3
    assert [r["status"] for r in res] == [0, 0, L.AICP_ERR_CONVERGENCE]
    assert res[2]["crop_points"] > 0 and not res[2]["accepted"]
    check_against_replay(oracle, mp, reads_bad, poses, origins, False, T, res, final,
                         cfg=oracle.default_config(nn_max_dist=5.0))
    with pytest.raises(L.ConvergenceError):
        run(ctx, mp, reads_bad, poses, prm, cfg=cfg)


def test_rows_of_16_bytes(ctx, L, world):
    mp, reads, poses, origins = world
    prm = params(L)
    T, res, done, rc, final = run(ctx, mp, reads[:5], poses[:5], prm)
    rows = [np.concatenate([r, np.full((len(r), 1), 7.0, np.float32)], 1) for r in reads[:5]]  # pcl::PointXYZ
    assert rows[0].shape[1] == 4
    T4, res4, done4, rc4, final4 = run(ctx, mp, rows, poses[:5], prm)
    assert rc == rc4 == 0 and done == done4 == 5
    np.testing.assert_array_equal(T, T4)
    assert res == res4
    np.testing.assert_array_equal(final, final4)
    assert sum(r["merged"] for r in res) == 2 and len(final) != len(mp)
