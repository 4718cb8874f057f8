"""Raw readings in the two map localization streams (aicp_hip_map_sequence_run_raw,
aicp_hip_built_map_sequence_run_raw; PriorMap / BuiltMap .sequence_run(raw=True)) and their ingest
kernel (aicp_hip_test_ingest) against the host restatement of tests/raw_stream_reference.py, against
the hand composition (aicp_hip_prefilter per reading, then the pre-filtered stream) and against
numpy. Fixtures and expected patterns: tests/test_raw_stream_cpu.py pins them on the CPU."""
import ctypes as C

import numpy as np
import pytest

import built_map_reference as bm
import localization_reference as lr
import raw_stream_reference as rs
from aicp_mapping_amd import synthetic as sy
from test_built_map_stream import check_record  # the built-map registration's comparisons, unchanged

pytestmark = pytest.mark.gpu

STREAMS = ["prior", "built"]
MODES = [False, True]
MODE_IDS = ["robot", "debug"]


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
def worlds(oracle):
    """stream -> (map, raw readings, poses, origins); read only."""
    return dict(prior=rs.prior_world(oracle), built=rs.built_world(oracle))


def params(L, stream, debug=False, **kw):
    if stream == "prior":
        return L.default_localization_params(**dict(lr.PARAMS, debug=debug, **kw))
    return L.default_built_map_params(**dict(bm.PARAMS, debug=debug, **kw))


def make_map(ctx, stream, pts):
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.prior_map import PriorMap

    return (PriorMap if stream == "prior" else BuiltMap)(ctx, pts)


def run_raw(ctx, L, stream, mp, raws, poses, debug=False, raise_on_error=True, read_prefilter=None):
    m = make_map(ctx, stream, mp)
    T, res, done, rc, kept = m.sequence_run(raws, poses, params=params(L, stream, debug), raw=True,
                                            read_prefilter=read_prefilter, raise_on_error=raise_on_error)
    final = m.getCloud()
    m.free()
    return dict(T=T, res=res, done=done, rc=rc, kept=[int(k) for k in kept], final=final)


def run_filtered(ctx, L, stream, mp, reads, poses, debug=False):
    m = make_map(ctx, stream, mp)
    T, res, done, rc = m.sequence_run(reads, poses, params=params(L, stream, debug))
    final = m.getCloud()
    m.free()
    return dict(T=T, res=res, done=done, rc=rc, final=final)


def replay(oracle, stream, world, debug, n=None, raws=None, poses=None, **kw):
    mp, r0, p0, origins = world
    raws, poses = raws or r0, poses or p0
    n = len(raws) if n is None else n
    if stream == "prior":
        return rs.replay_prior_raw(oracle, mp, raws[:n], poses[:n], origins[:n], debug=debug, **dict(lr.PARAMS, **kw))
    return rs.replay_built_raw(oracle, mp, raws[:n], poses[:n], origins[:n], debug=debug, **dict(bm.PARAMS, **kw))


APPEND = dict(prior="merged", built="is_reference")


def check_against_replay(oracle, stream, world, debug, out, raws=None, poses=None):
    """As check_against_replay of tests/test_localization_stream.py / tests/test_built_map_stream.py,
    with the raw replays and the kept counts: the free-running replay takes the same decisions; the
    forced replay (state from the device's corrections) keeps the same points of every reading,
    sees the same maps and crops (built map: the same overlap keys and ratio), registers in the same
    iterations with the same NN touch counts, and ends with the same map, bit for bit."""
    T, res = out["T"], out["res"]
    n = len(res)
    flags = ("status", "accepted", APPEND[stream]) + (("refiltered",) if stream == "prior" else ())
    free, _ = replay(oracle, stream, world, debug, n, raws, poses)
    for k in flags:
        assert [r[k] for r in res] == [r[k] for r in free], k
    forced, fmap = replay(oracle, stream, world, debug, n, raws, poses, forced_T=T)
    assert out["kept"][:n] == [r["kept"] for r in forced]
    assert out["kept"][n:] == [0] * (len(out["kept"]) - n)
    for i, (d, r) in enumerate(zip(res, forced)):
        for k in flags + ("map_points", "crop_points"):
            assert d[k] == r[k], (i, k, d[k], r[k])
        if r["status"]:
            continue
        if stream == "built":
            check_record(i, d["icp"], r, T[i])
        else:
            assert d["icp"]["iterations"] == r["stats"].iterations, i
            assert (d["icp"]["nn_points_touched"], d["icp"]["nn_nodes_touched"]) == (r["stats"].nn_points_touched,
                                                                                   r["stats"].nn_nodes_touched), i
            assert d["icp"]["trimmed_ratio"] == np.float32(0.5)
            rr, tt = sy.rot_err(r["T"], T[i])
            assert rr < 1e-6 and tt < 1e-5, (i, rr, tt)
        if r["accepted"]:
            np.testing.assert_allclose(d["corrected_origin"], r["corrected_origin"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(out["final"], fmap)
    return forced


@pytest.fixture(scope="module")
def runs(ctx, L, worlds):
    """(stream, debug) -> the raw stream's results on the fixture, each run once (read only)."""
    cache = {}

    def get(stream, debug):
        if (stream, debug) not in cache:
            mp, raws, poses, _ = worlds[stream]
            cache[(stream, debug)] = run_raw(ctx, L, stream, mp, raws, poses, debug)
        return cache[(stream, debug)]

    return get


# ---- 1. against the replay ---------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_raw_stream_equals_replay(oracle, worlds, runs, stream, debug):
    out = runs(stream, debug)
    n = len(worlds[stream][1])
    assert out["rc"] == 0 and out["done"] == n
    check_against_replay(oracle, stream, worlds[stream], debug, out)
    res = out["res"]
    if stream == "prior":
        assert [r["accepted"] for r in res] == [1, 1, 0, 1, 1, 0, 1, 1]
        assert [i for i, r in enumerate(res) if r["merged"]] == [0, 4]
        assert [i for i, r in enumerate(res) if r["refiltered"]] == [0, 6]
    else:
        assert [r["accepted"] for r in res] == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
        assert [i for i, r in enumerate(res) if r["is_reference"]] == [2, 6, 9]


# ---- 2. robot mode is the hand composition, bit for bit --------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_robot_mode_equals_hand_composition(ctx, L, worlds, runs, stream):
    mp, raws, poses, _ = worlds[stream]
    out = runs(stream, False)
    kept = [ctx.prefilter(r) for r in raws]  # every kept cloud to the host, then uploaded again
    exp = run_filtered(ctx, L, stream, mp, kept, poses)
    assert out["kept"] == [len(k) for k in kept]
    assert np.array_equal(out["T"], exp["T"])
    assert (out["rc"], out["done"]) == (exp["rc"], exp["done"]) == (0, len(raws))
    assert out["res"] == exp["res"]
    assert np.array_equal(out["final"], exp["final"])


@pytest.mark.parametrize("stream", STREAMS)
def test_point_to_point_chain_equals_hand_composition(ctx, L, worlds, stream):
    """knn_normals = 0 (PointToPointErrorMinimizer) runs through the raw streams as through the
    pre-filtered ones."""
    mp, raws, poses, _ = worlds[stream]
    n = 4
    cfg = L.default_config(knn_normals=0)
    m = make_map(ctx, stream, mp)
    T, res, done, rc, kept = m.sequence_run(raws[:n], poses[:n], cfg=cfg, params=params(L, stream), raw=True)
    final = m.getCloud()
    m.free()
    filtered = [ctx.prefilter(r) for r in raws[:n]]
    m = make_map(ctx, stream, mp)
    Te, rese, donee, rce = m.sequence_run(filtered, poses[:n], cfg=cfg, params=params(L, stream))
    finale = m.getCloud()
    m.free()
    assert (rc, done) == (rce, donee) == (0, n) and [int(k) for k in kept] == [len(f) for f in filtered]
    assert np.array_equal(T, Te) and res == rese and np.array_equal(final, finale)


# ---- 3. debug mode keeps App's points, not the swapped order's -------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_debug_mode_keeps_apps_counts(oracle, worlds, runs, stream):
    out = runs(stream, True)
    app, _ = replay(oracle, stream, worlds[stream], True, forced_T=out["T"])
    swp, _ = replay(oracle, stream, worlds[stream], True, forced_T=out["T"], order="swapped")
    ka, ks = [r["kept"] for r in app], [r["kept"] for r in swp]
    assert out["kept"] == ka
    assert ka[0] == ks[0] and all(a != s for a, s in zip(ka[1:], ks[1:])), (ka, ks)


# ---- 4. a reading the pre-filter empties -----------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_an_emptied_reading_ends_the_stream(ctx, oracle, L, worlds, stream, debug):
    mp, raws, poses, _ = worlds[stream]
    bad = raws[:3] + [rs.scattered()] + raws[4:]
    out = run_raw(ctx, L, stream, mp, bad, poses, debug, raise_on_error=False)
    assert out["rc"] == L.AICP_ERR_INVALID and out["done"] == 4 and len(out["res"]) == 4
    assert [r["status"] for r in out["res"]] == [0, 0, 0, L.AICP_ERR_INVALID]
    assert out["res"][3]["icp"]["status"] == L.AICP_ERR_INVALID and not out["res"][3]["accepted"]
    assert np.array_equal(out["T"][3], np.eye(4, dtype=np.float32))
    assert out["kept"][3:] == [0] * (len(raws) - 3) and all(k > 0 for k in out["kept"][:3])
    assert "reading 3" in ctx.last_error() and "pre-filter" in ctx.last_error()
    # readings 0-2 as the replay's, and the map as after reading 2
    check_against_replay(oracle, stream, worlds[stream], debug, out, raws=bad)
    good = run_raw(ctx, L, stream, mp, raws[:3], poses[:3], debug)
    assert np.array_equal(out["T"][:3], good["T"]) and out["res"][:3] == good["res"]
    assert np.array_equal(out["final"], good["final"])
    with pytest.raises(L.AicpError) as e:
        run_raw(ctx, L, stream, mp, bad, poses, debug)
    assert e.value.code == L.AICP_ERR_INVALID


def test_of_an_empty_crop_and_an_emptied_reading_the_lower_index_wins(ctx, oracle, L, worlds):
    """Readings 1-3 of the prior-map fixture are one window in robot mode."""
    mp, raws, poses, _ = worlds["prior"]
    far = np.array(poses[2], np.float64)
    far[:3, 3] += (200.0, 0.0, 0.0)
    # the crop of reading 2 is empty, reading 3 is emptied
    r_a, p_a = raws[:3] + [rs.scattered()] + raws[4:], poses[:2] + [far] + poses[3:]
    a = run_raw(ctx, L, "prior", mp, r_a, p_a, raise_on_error=False)
    assert a["rc"] == L.AICP_ERR_INVALID and a["done"] == 3 and "empty map crop" in ctx.last_error()
    assert a["kept"][2] > 0 and a["kept"][3:] == [0] * 5 and a["res"][2]["crop_points"] == 0
    check_against_replay(oracle, "prior", worlds["prior"], False, a, raws=r_a, poses=p_a)
    # reading 2 is emptied, the crop of reading 3 is empty
    far3 = np.array(poses[3], np.float64)
    far3[:3, 3] += (200.0, 0.0, 0.0)
    r_b, p_b = raws[:2] + [rs.scattered()] + raws[3:], poses[:3] + [far3] + poses[4:]
    b = run_raw(ctx, L, "prior", mp, r_b, p_b, raise_on_error=False)
    assert b["rc"] == L.AICP_ERR_INVALID and b["done"] == 3 and "pre-filter" in ctx.last_error()
    assert b["kept"][2:] == [0] * 6
    check_against_replay(oracle, "prior", worlds["prior"], False, b, raws=r_b, poses=p_b)
    assert np.array_equal(a["T"][:2], b["T"][:2]) and np.array_equal(a["final"], b["final"])


# ---- 5. row widths -----------------------------------------------------------------------------------
def widen(r, w, fill):
    return np.concatenate([r, np.full((len(r), w - 3), fill, np.float32)], 1)


@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_rows_of_12_16_and_32_bytes(ctx, L, worlds, stream, debug):
    mp, raws, poses, _ = worlds[stream]
    n = 5 if stream == "prior" else 4  # past the first merge / append and a dropped reading
    base = run_raw(ctx, L, stream, mp, raws[:n], poses[:n], debug)
    assert base["rc"] == 0 and base["done"] == n
    assert sum(r[APPEND[stream]] for r in base["res"]) >= 1 and 0 in [r["accepted"] for r in base["res"]]
    for w, fill in ((4, 7.0), (8, np.nan)):  # pcl::PointXYZ (verbatim), PointXYZRGB (packed on the host)
        rows = [widen(r, w, fill) for r in raws[:n]]
        out = run_raw(ctx, L, stream, mp, rows, poses[:n], debug)
        assert (out["rc"], out["done"], out["kept"]) == (0, n, base["kept"]), w
        assert np.array_equal(out["T"], base["T"]), w
        assert out["res"] == base["res"], w
        assert np.array_equal(out["final"], base["final"]), w


# ---- 6. the ingest kernel alone ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ingest_points():
    g = np.random.default_rng(5)
    p = (g.standard_normal((70001, 3)) * np.float32(20.0)).astype(np.float32)
    p[3] = (np.nan, 1.0, -np.inf)  # a non-finite point passes through
    p[70000] = (np.inf, np.nan, 0.0)
    return p


@pytest.mark.parametrize("stride", [12, 16, 32, 48])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_ingest_kernel(ctx, ingest_points, n, stride):
    pts = ingest_points[70001 - n:] if n < 4 else ingest_points[:n]
    rows = widen(pts, stride // 4, -3.0) if stride > 12 else pts
    out = ctx.test_ingest(rows)
    exp = np.concatenate([pts, np.ones((n, 1), np.float32)], 1)
    assert out.shape == (n, 4)
    assert np.array_equal(out.view(np.uint32), exp.view(np.uint32))  # bit for bit, NaN and inf included
    T = sy.make_T(yaw_deg=17.0, pitch_deg=-3.0, roll_deg=5.0, t=(0.4, -1.3, 0.2)).astype(np.float32)
    fin = np.isfinite(pts).all(1)
    moved = ctx.test_ingest(rows, T)
    ref = ctx.transform(T, pts)
    assert np.array_equal(moved[fin, :3].view(np.uint32), ref[fin].view(np.uint32))
    assert np.array_equal(moved[:, 3], np.ones(n, np.float32))
    assert not np.isfinite(moved[~fin, :3]).all(1).any()


# ---- 7. argument checks ------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_argument_checks(ctx, L, worlds, stream):
    from aicp_mapping_amd.prior_map import _clouds_and_poses

    mp, raws, poses, _ = worlds[stream]
    m = make_map(ctx, stream, mp)
    n = 2
    arr, pz, keep = _clouds_and_poses(raws[:n], poses[:n])
    cfg, prm, pf = L.default_config(), params(L, stream), L.default_prefilter()
    outT = np.full((n, 16), 9.0, np.float32)
    res = ((L.LocalizationResult if stream == "prior" else L.BuiltMapResult) * n)()
    kept = np.full(n, 9, np.uint32)

    def call(pf_read, n_readings=n, with_done=True):
        done = C.c_size_t(77)
        pfr = C.byref(pf_read) if pf_read is not None else None
        tail = (m.h, arr, L._fptr(pz), n_readings, L._fptr(outT), res, kept.ctypes.data_as(C.POINTER(C.c_uint32)),
                C.byref(done) if with_done else None)
        if stream == "prior":
            rc = L.lib.aicp_hip_map_sequence_run_raw(ctx.h, C.byref(cfg), C.byref(prm), None, pfr, *tail)
        else:
            rc = L.lib.aicp_hip_built_map_sequence_run_raw(ctx.h, C.byref(cfg), C.byref(prm), pfr, *tail)
        return rc, done.value

    def untouched():
        assert len(m) == len(mp) and np.array_equal(m.getCloud(), mp)
        assert (outT == 9.0).all() and all(r.status == 0 and r.map_points == 0 for r in res)

    assert call(None) == (L.AICP_ERR_INVALID, 0)
    untouched()
    assert call(L.default_prefilter(normal_k=25)) == (L.AICP_ERR_UNSUPPORTED, 0)
    untouched()
    assert call(pf, with_done=False) == (L.AICP_ERR_INVALID, 77)
    untouched()
    assert call(pf, n_readings=0) == (L.AICP_OK, 0)
    untouched()
    m.free()


# ---- 8. one context across the streams ---------------------------------------------------------------
def test_one_context_serves_the_streams_in_turn(L, worlds):
    """Raw prior map, pre-filtered prior map, raw built map on one context (the pre-filter, the crop
    and the batch share its buffers): each as the same call on a fresh context, bit for bit."""
    pmap, praws, pposes, _ = worlds["prior"]
    first, braws, bposes, _ = worlds["built"]
    n = 5
    c0 = L.Context(0)
    kept = [c0.prefilter(r) for r in praws[:n]]
    calls = [lambda c: run_raw(c, L, "prior", pmap, praws[:n], pposes[:n], True),
             lambda c: run_filtered(c, L, "prior", pmap, kept, pposes[:n]),
             lambda c: run_raw(c, L, "built", first, braws[:n], bposes[:n], False)]
    shared = [f(c0) for f in calls]
    c0.close()
    for f, a in zip(calls, shared):
        c = L.Context(0)
        b = f(c)
        c.close()
        assert a["rc"] == b["rc"] == 0 and a["done"] == b["done"] == n
        assert np.array_equal(a["T"], b["T"])
        assert a["res"] == b["res"] and a.get("kept") == b.get("kept")
        assert np.array_equal(a["final"], b["final"])
