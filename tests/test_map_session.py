"""The live map sessions (aicp_hip_map_session_*; MapSession): one reading per call on the prior map
or on the built map, against the host restatements of tests/raw_stream_reference.py,
tests/localization_reference.py and tests/built_map_reference.py, against the offline streams whose
rules they state reading by reading, and the device-decided append against ctx.transform.
Fixtures and expected patterns: tests/test_raw_stream_cpu.py and tests/test_map_session_cpu.py pin
them on the CPU."""
import ctypes as C

import numpy as np
import pytest

import built_map_reference as bm
import localization_reference as lr
import raw_stream_reference as rs
from aicp_mapping_amd import synthetic as sy
from test_built_map_stream import check_against_replay as check_built_filtered
from test_localization_stream import check_against_replay as check_prior_filtered
from test_raw_stream import APPEND, check_against_replay, make_map, params  # the raw streams' comparisons, unchanged
from test_session import scene_sweeps

pytestmark = pytest.mark.gpu

STREAMS = ["prior", "built"]
MODES = [False, True]
MODE_IDS = ["robot", "debug"]
F32 = np.float32
FREQ1 = dict(reference_update_frequency=1)


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


@pytest.fixture(scope="module")
def filtered_worlds(oracle):
    """stream -> (map, pre-filtered readings, poses, origins) of the pre-filtered streams' tests."""
    return dict(prior=(lr.make_map(oracle),) + lr.make_stream(10, lr.JUMPS),
                built=(bm.make_first_cloud(oracle),) + bm.make_stream())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def session(ctx, L, stream, m, debug=False, raw=True, cfg=None, **kw):
    from aicp_mapping_amd.map_session import MapSession

    return MapSession(ctx, m, cfg=cfg, params=params(L, stream, debug, **kw), prefilter=True if raw else None)


def feed(ctx, L, stream, mp, reads, poses, debug=False, raw=True, cfg=None, between=None, **kw):
    """The readings one by one through a session on a fresh map; the result in the shape of
    test_raw_stream.run_raw's (T and res of the readings processed, kept padded with zeros)."""
    m = make_map(ctx, stream, mp)
    s = session(ctx, L, stream, m, debug, raw, cfg, **kw)
    s.start()
    out = dict(T=[], res=[], kept=[], rc=0, sizes=[])
    for i, (r, P) in enumerate(zip(reads, poses)):
        T, d, k = s.process(r, P, raise_on_error=False)
        out["rc"] = d.pop("rc")
        out["T"].append(T)
        out["res"].append(d)
        out["kept"].append(k)
        out["sizes"].append(len(m))  # (map->n is final when process returns)
        if out["rc"]:
            break
        if between:
            between(i, m)
    out["done"] = len(out["res"])
    out["kept"] += [0] * (len(reads) - out["done"])
    out["T"] = np.array(out["T"], F32).reshape(-1, 4, 4)
    out["final"] = m.getCloud()
    out["state"] = s.state()
    out["error"] = ctx.last_error()
    s.close()
    m.free()
    return out


def stream_run(ctx, L, stream, mp, reads, poses, debug=False, raw=True, cfg=None, **kw):
    """The offline stream on a fresh map, in the same shape."""
    m = make_map(ctx, stream, mp)
    r = m.sequence_run(reads, poses, cfg=cfg, params=params(L, stream, debug, **kw), raw=raw, raise_on_error=False)
    T, res, done, rc = r[:4]
    kept = [int(k) for k in r[4]] if raw else [len(x) for x in reads[:done]] + [0] * (len(reads) - done)
    out = dict(T=T[:done], res=res, done=done, rc=rc, kept=kept, final=m.getCloud(), error=ctx.last_error())
    m.free()
    return out


def assert_same_run(a, b, kept=True):
    assert (a["rc"], a["done"]) == (b["rc"], b["done"])
    if kept:
        assert a["kept"] == b["kept"]
    assert same_bits(a["T"], b["T"])
    for i, (x, y) in enumerate(zip(a["res"], b["res"])):
        assert x == y, i
    assert same_bits(a["final"], b["final"])


def assert_same_decisions(a, b, stream):
    """What a batched window may not change: every decision and count, the final map's size; T at
    the replay's tolerances (1e-6 rad, 1e-5 m)."""
    assert (a["rc"], a["done"], a["kept"]) == (b["rc"], b["done"], b["kept"])
    keys = ("status", "accepted", APPEND[stream], "map_points", "crop_points") + (
        ("refiltered",) if stream == "prior" else ())
    for i, (x, y) in enumerate(zip(a["res"], b["res"])):
        for k in keys:
            assert x[k] == y[k], (i, k)
        rr, tt = sy.rot_err(a["T"][i], b["T"][i])
        assert rr < 1e-6 and tt < 1e-5, (i, rr, tt)
    assert len(a["final"]) == len(b["final"])


def assert_pattern(stream, res):
    if stream == "prior":
        assert [r["accepted"] for r in res] == [1, 1, 0, 1, 1, 0, 1, 1]
        assert [i for i, r in enumerate(res) if r["merged"]] == [0, 4]
        assert [i for i, r in enumerate(res) if r["refiltered"]] == [0, 6]
    else:
        assert [r["accepted"] for r in res] == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
        assert [i for i, r in enumerate(res) if r["is_reference"]] == [2, 6, 9]


@pytest.fixture(scope="module")
def runs(ctx, L, worlds):
    """(stream, debug) -> the session's results on the raw fixture, each run once (read only)."""
    cache = {}

    def get(stream, debug):
        if (stream, debug) not in cache:
            mp, raws, poses, _ = worlds[stream]
            cache[(stream, debug)] = feed(ctx, L, stream, mp, raws, poses, debug)
        return cache[(stream, debug)]

    return get


# ---- 1. against the replay ---------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_session_equals_replay(oracle, worlds, runs, stream, debug):
    out = runs(stream, debug)
    n = len(worlds[stream][1])
    assert out["rc"] == 0 and out["done"] == n
    check_against_replay(oracle, stream, worlds[stream], debug, out)
    assert_pattern(stream, out["res"])
    # the map's size after every call is the next reading's map_points, and the final map's
    assert out["sizes"] == [r["map_points"] for r in out["res"][1:]] + [len(out["final"])]
    st = out["state"]
    assert st["n_processed"] == n and not st["ended"]
    accepted = [r["accepted"] for r in out["res"]]
    assert st["count"] == (sum(accepted) if stream == "prior" else 0)  # (built: reading 9 is a reference)
    assert not np.array_equal(st["initial_T"], np.eye(4, dtype=F32))


# ---- 2. debug mode is the stream, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_debug_mode_equals_the_stream(ctx, L, worlds, runs, stream):
    mp, raws, poses, _ = worlds[stream]
    assert_same_run(runs(stream, True), stream_run(ctx, L, stream, mp, raws, poses, True))


# ---- 3. robot mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_robot_mode_at_frequency_1_equals_the_stream(ctx, L, worlds, stream):
    """Every window of the stream is one reading long, so it is the session's call, bit for bit; the
    pattern is the one tests/test_map_session_cpu.py pins on the replay."""
    mp, raws, poses, _ = worlds[stream]
    out = feed(ctx, L, stream, mp, raws, poses, False, **FREQ1)
    assert_same_run(out, stream_run(ctx, L, stream, mp, raws, poses, False, **FREQ1))
    accepted = [r["accepted"] for r in out["res"]]
    assert out["rc"] == 0 and accepted.count(0) >= 1
    assert [r[APPEND[stream]] for r in out["res"]] == accepted
    if stream == "prior":
        assert accepted == [1, 1, 0, 1, 1, 0, 1, 1]
        assert [i for i, r in enumerate(out["res"]) if r["refiltered"]] == [0, 6]


@pytest.mark.parametrize("stream", STREAMS)
def test_robot_mode_at_the_fixtures_frequency_decides_as_the_stream(ctx, L, worlds, runs, stream):
    """The stream batches the readings between two map changes; the session runs them one by one."""
    mp, raws, poses, _ = worlds[stream]
    out, exp = runs(stream, False), stream_run(ctx, L, stream, mp, raws, poses, False)
    assert_same_decisions(out, exp, stream)
    print("map session, %s, robot mode at the fixture's frequency: T bits %s, result records %s, final map bits %s"
          % (stream, same_bits(out["T"], exp["T"]), out["res"] == exp["res"], same_bits(out["final"], exp["final"])))


# ---- 4. the pre-filtered entry -------------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_prefiltered_readings(ctx, oracle, L, filtered_worlds, stream, debug):
    mp, reads, poses, origins = filtered_worlds[stream]
    out = feed(ctx, L, stream, mp, reads, poses, debug, raw=False)
    assert out["rc"] == 0 and out["done"] == len(reads) == 10
    assert out["kept"] == [len(r) for r in reads]
    if stream == "prior":
        check_prior_filtered(oracle, mp, reads, poses, origins, debug, out["T"], out["res"], out["final"])
    else:
        check_built_filtered(oracle, mp, reads, poses, origins, params(L, stream, debug), out["T"], out["res"],
                             out["final"])
    assert sum(r[APPEND[stream]] for r in out["res"]) >= 2
    if not (stream == "built" and debug):  # (there the moved reading 4 registers within the limit: the replay too)
        assert [r["accepted"] for r in out["res"]].count(0) >= 1
    exp = stream_run(ctx, L, stream, mp, reads, poses, debug, raw=False)
    if debug:  # the stream's windows are one reading long
        assert_same_run(out, exp)
    else:
        assert_same_decisions(out, exp, stream)


# ---- 5. the append's edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
def test_the_append_at_its_edges(ctx, oracle, L, debug):
    """Readings of 1023, 1024, 1025 and 4097 points behind a map of 3001 (its tail starts off any
    tile boundary) that has room for its cloud only: after every call the map is the map before
    followed by the reading as registered, moved by its correction; after a dropped reading it is
    the map before."""
    from aicp_mapping_amd.prior_map import PriorMap

    full = lr.make_map(oracle)
    mp = full[np.linspace(0, len(full) - 1, 3001).astype(np.int64)]
    sizes = [1023, 1024, 3000, 1025, 4097]
    rd = [lr.make_reading(i, n_points=n, jump=lr.JUMPS.get(i)) for i, n in enumerate(sizes)]  # (reading 2 jumps)
    m = PriorMap(ctx, mp)
    assert len(m) == m.capacity == 3001
    s = session(ctx, L, "prior", m, debug, raw=False, map_refilter_every=0, **FREQ1)
    s.start()
    accepted = []
    for i, (r, P) in enumerate(rd):
        assert len(r) == sizes[i]
        before, initT = m.getCloud(), s.state()["initial_T"]
        T, d, kept = s.process(r, P)
        accepted.append(d["accepted"])
        assert d["status"] == 0 and kept == len(r) and d["map_points"] == len(before) and not d["refiltered"]
        assert d["merged"] == d["accepted"]
        registered = ctx.transform(initT, r) if debug else r
        exp = np.concatenate([before, ctx.transform(T, registered)], 0) if d["merged"] else before
        assert len(m) == len(exp), i
        assert same_bits(m.getCloud(), exp), i
        if i == 0:
            assert m.capacity >= 3001 + 1023  # grown, by copy
    assert accepted == [1, 1, 0, 1, 1]
    assert len(m) == 3001 + 1023 + 1024 + 1025 + 4097
    s.close()
    m.free()


# ---- 6. readings from the sweep accumulator ------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_readings_from_the_accumulator(ctx, L, stream, debug):
    """process(acc, pose) reads the accumulator's cloud where it lies: the same bits as
    process(acc.getCloud(), pose) by a twin session on a twin map, the accumulator unchanged and free
    to be cleared and refilled at once."""
    from aicp_mapping_amd.accumulator import SweepAccumulator

    def fill(acc, k):
        sweeps, poses = scene_sweeps(k)
        for sw, P in zip(sweeps, poses):
            acc.push(sw, P)
        # (the accumulator entry takes the pose in float and the origin from it: a pose that float holds)
        return np.asarray(poses[1], F32).astype(np.float64)

    cap = max(sum(len(s) for s in scene_sweeps(k)[0]) for k in range(4))
    acc = SweepAccumulator(ctx, cap, batch_size=3)
    fill(acc, 0)
    first = ctx.prefilter(acc.getCloud())
    assert len(first) >= 50
    kw = dict(reference_update_frequency=1 if stream == "prior" else 2, max_correction_magnitude=1.0)
    ma, mb = make_map(ctx, stream, first), make_map(ctx, stream, first)
    a, b = session(ctx, L, stream, ma, debug, **kw), session(ctx, L, stream, mb, debug, **kw)
    a.start()
    b.start()
    appended = 0
    for k in (1, 2, 3):
        acc.clear()
        P = fill(acc, k)
        cloud = acc.getCloud()
        Ta, ra, ka = a.process(acc, P)
        assert same_bits(acc.getCloud(), cloud)  # left as it is
        acc.clear()
        fill(acc, (k + 1) % 4)  # the node's next reading starts at once
        Tb, rb, kb = b.process(cloud, P)
        assert same_bits(Ta, Tb) and ra == rb and ka == kb, k
        assert ra["status"] == 0 and ra["accepted"] == 1 and 50 <= ka < len(cloud)
        appended += ra[APPEND[stream]]
        sa, sb = a.state(), b.state()
        assert same_bits(sa["initial_T"], sb["initial_T"]) and sa["count"] == sb["count"]
        assert len(ma) == len(mb)
    assert appended >= 1 and len(ma) > len(first)
    assert same_bits(ma.getCloud(), mb.getCloud())
    for x in (a, b):
        x.close()
    for m in (ma, mb, acc):
        m.free()


def test_the_accumulator_needs_a_prefilter(ctx, L, worlds):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    mp, raws, poses, _ = worlds["prior"]
    sweeps, sp = scene_sweeps(1)
    acc = SweepAccumulator(ctx, sum(len(s) for s in sweeps), batch_size=3)
    acc.push(sweeps[0], sp[0])
    m = make_map(ctx, "prior", mp)
    s = session(ctx, L, "prior", m, raw=False)
    s.start()
    T, d, kept = s.process(acc, poses[0], raise_on_error=False)
    assert d["rc"] == L.AICP_ERR_INVALID and "pf_read" in ctx.last_error()
    st = s.state()
    assert not st["ended"] and st["n_processed"] == 0  # an argument error, not a reading
    s.close()
    m.free()
    acc.free()


# ---- 7. isolation ----------------------------------------------------------------------------------------
def test_other_calls_between_readings_change_nothing(ctx, L, worlds, runs):
    mp, raws, poses, _ = worlds["prior"]
    other = sy.make_pair(3000, 3000, seed=5)
    seen = []

    def between(i, m):
        if i % 2 == 1:
            ctx.register(other.ref, other.read)
        ctx.overlap(other.ref, other.read, other.ref_origin, other.read_origin)
        ctx.prefilter(raws[(i + 3) % len(raws)])
        crop = m.crop(-6.0, 6.0, poses[i])
        seen.append((len(crop), len(m.getCloud())))

    out = feed(ctx, L, "prior", mp, raws, poses, True, between=between)
    assert_same_run(out, runs("prior", True))
    assert [n for _, n in seen] == out["sizes"] and all(c > 0 for c, _ in seen)


def test_sessions_interleaved_on_one_context(ctx, L, worlds, runs):
    """A prior-map session, a built-map session and an AppSession fed in turn each equal their solo
    run."""
    from aicp_mapping_amd.session import AppSession

    pmp, praws, pposes, _ = worlds["prior"]
    bmp, braws, bposes, _ = worlds["built"]
    n = 6
    st = sy.make_stream(n_readings=n, n_points=3000, seed=8, half=18.0)

    def app_session():
        s = AppSession(ctx, params=L.default_sequence_params(reference_update_frequency=2))
        s.start(st.first, st.first_origin)
        return s

    def app_step(s, i):
        T, d, k = s.process(st.readings[i], st.origins[i])
        return T, d, k

    x = app_session()
    solo = [app_step(x, i) for i in range(n)]
    x.close()
    pm, bmm = make_map(ctx, "prior", pmp), make_map(ctx, "built", bmp)
    p, b, x = session(ctx, L, "prior", pm, True), session(ctx, L, "built", bmm, False), app_session()
    p.start()
    b.start()
    for i in range(n):
        Tp, dp, kp = p.process(praws[i], pposes[i])
        Tb, db, kb = b.process(braws[i], bposes[i])
        Tx, dx, kx = app_step(x, i)
        for (T, d, k), run in (((Tp, dp, kp), runs("prior", True)), ((Tb, db, kb), runs("built", False))):
            d.pop("rc")
            assert same_bits(T, run["T"][i]) and d == run["res"][i] and k == run["kept"][i], i
        assert same_bits(Tx, solo[i][0]) and dx == solo[i][1] and kx == solo[i][2], i
    assert [len(pm), len(bmm)] == [runs("prior", True)["sizes"][n - 1], runs("built", False)["sizes"][n - 1]]
    for s in (p, b, x):
        s.close()
    pm.free()
    bmm.free()


# ---- 8. endings --------------------------------------------------------------------------------------------
def ending_inputs(kind, raws, poses):
    if kind == "crop":
        far = np.array(poses[3], np.float64)
        far[:3, 3] += (200.0, 0.0, 0.0)
        return raws, poses[:3] + [far] + poses[4:], None
    if kind == "emptied":
        return raws[:3] + [rs.scattered()] + raws[4:], poses, None
    shifted = (raws[3] + F32([200.0, 0.0, 0.0])).astype(F32)  # nothing within nn_max_dist: no convergence
    return raws[:3] + [shifted] + raws[4:], poses, dict(nn_max_dist=5.0)


@pytest.mark.parametrize("kind", ["crop", "emptied", "registration"])
@pytest.mark.parametrize("stream", STREAMS)
def test_what_ends_a_session(ctx, L, worlds, stream, kind):
    mp, raws, poses, _ = worlds[stream]
    raws, poses, cfg_kw = ending_inputs(kind, raws, poses)
    cfg = L.default_config(**cfg_kw) if cfg_kw else None
    m = make_map(ctx, stream, mp)
    s = session(ctx, L, stream, m, False, cfg=cfg)
    s.start()
    for i in range(3):
        T, d, k = s.process(raws[i], poses[i])
        assert d["status"] == 0
    st0, map0 = s.state(), m.getCloud()
    T, d, k = s.process(raws[3], poses[3], raise_on_error=False)
    err = ctx.last_error()
    # the stream's record of the reading that ends it, and its status
    exp = stream_run(ctx, L, stream, mp, raws, poses, False, cfg=cfg)
    code = exp["rc"]
    assert (code == L.AICP_ERR_INVALID) == (kind != "registration") and code != 0 and exp["done"] == 4
    assert d["rc"] == d["status"] == code and not d["accepted"] and not d[APPEND[stream]]
    assert "reading 3" in err
    assert {"crop": "empty map crop", "emptied": "pre-filter", "registration": "status"}[kind] in err
    d.pop("rc")
    assert d == exp["res"][3] and same_bits(T, exp["T"][3])
    assert k == exp["kept"][3] and (k == 0) == (kind == "emptied")
    if kind != "registration":
        # (an emptied reading is looked at before its crop: no crop either)
        assert same_bits(T, np.eye(4, dtype=F32)) and d["crop_points"] == 0 and d["map_points"] == len(map0)
    # the map and the state are as before the call
    st1 = s.state()
    assert st1["ended"] and st1["n_processed"] == 4 and st1["count"] == st0["count"]
    assert same_bits(st1["initial_T"], st0["initial_T"])
    assert len(m) == len(map0) and same_bits(m.getCloud(), map0)
    # ended: further readings are refused, until start
    T, d, k = s.process(raws[4], poses[4], raise_on_error=False)
    assert d["rc"] == L.AICP_ERR_INVALID and "ended at reading 3" in ctx.last_error()
    with pytest.raises(L.AicpError):
        s.process(raws[4], poses[4])
    assert s.state()["n_processed"] == 4
    s.start()
    st2 = s.state()
    assert not st2["ended"] and st2["n_processed"] == 0 and st2["count"] == 0
    assert same_bits(st2["initial_T"], np.eye(4, dtype=F32))
    T, d, k = s.process(raws[4], poses[4])
    assert d["status"] == 0 and s.state()["n_processed"] == 1
    s.close()
    m.free()


def test_the_first_reading_on_the_prior_map_is_never_dropped(ctx, L, worlds):
    """lr.JUMP_ON_0: a first reading whose correction exceeds the limit is accepted on the prior
    map (getNbClouds() == 0) and dropped on the built map; start() makes a reading the first again."""
    reads, poses, _ = lr.make_stream(2, lr.JUMP_ON_0)  # (pre-filtered, as the streams' tests of the same rule)
    for stream, first_accepted in (("prior", 1), ("built", 0)):
        mp = worlds[stream][0]
        m = make_map(ctx, stream, mp)
        s = session(ctx, L, stream, m, False, raw=False)
        for _ in range(2):
            s.start()
            out = [s.process(r, P) for r, P in zip(reads, poses)]
            res = [d for _, d, _ in out]
            assert [d["status"] for d in res] == [0, 0]
            assert abs(out[0][0][1, 3]) > 0.4  # beyond max_correction_magnitude
            assert [d["accepted"] for d in res] == [first_accepted, 1]
            assert s.state()["count"] == 1 + first_accepted
        s.close()
        m.free()


# ---- 9. point-to-point chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_point_to_point_chain_equals_the_stream(ctx, L, worlds, stream):
    mp, raws, poses, _ = worlds[stream]
    n = 4
    cfg = L.default_config(knn_normals=0)
    out = feed(ctx, L, stream, mp, raws[:n], poses[:n], True, cfg=cfg)
    exp = stream_run(ctx, L, stream, mp, raws[:n], poses[:n], True, cfg=cfg)
    assert out["rc"] == 0 and out["done"] == n
    assert_same_run(out, exp)


# ---- 10. arguments --------------------------------------------------------------------------------------------
def test_create_refuses(ctx, L):
    cfg, loc, bmp, pf = L.default_config(), L.default_localization_params(), L.default_built_map_params(), \
        L.default_prefilter()
    bad, lib = L.AICP_ERR_INVALID, L.lib

    def create(cfg_, loc_, bm_, pf_read=None, pf_map=None, with_out=True):
        h = C.c_void_p(77)
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        rc = lib.aicp_hip_map_session_create(ctx.h, ref(cfg_), ref(loc_), ref(bm_), ref(pf_read), ref(pf_map),
                                             C.byref(h) if with_out else None)
        if rc == 0:
            lib.aicp_hip_map_session_free(ctx.h, h)
        else:
            assert with_out is False or h.value is None
        return rc

    assert create(cfg, loc, bmp) == bad  # both
    assert create(cfg, None, None) == bad  # neither
    assert create(cfg, None, bmp, pf_map=pf) == bad  # the built map is never re-filtered
    assert create(None, loc, None) == bad
    assert create(cfg, loc, None, with_out=False) == bad
    assert create(cfg, loc, None, pf_read=L.default_prefilter(normal_k=25)) == L.AICP_ERR_UNSUPPORTED
    assert create(cfg, None, bmp, pf_read=L.default_prefilter(normal_k=25)) == L.AICP_ERR_UNSUPPORTED
    assert create(cfg, L.default_localization_params(reference_update_frequency=0), None) == bad
    assert create(cfg, None, L.default_built_map_params(resolution=0.0)) == bad
    assert create(cfg, loc, None, pf_read=pf, pf_map=pf) == 0
    assert create(cfg, None, bmp, pf_read=pf) == 0
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.map_session import MapSession

    m = BuiltMap(ctx, np.zeros((4, 3), F32))
    with pytest.raises(TypeError):
        MapSession(ctx, m, params=loc)
    m.free()


@pytest.mark.parametrize("stream", STREAMS)
def test_argument_checks(ctx, L, worlds, stream):
    mp, raws, poses, _ = worlds[stream]
    m = make_map(ctx, stream, mp)
    s = session(ctx, L, stream, m)
    lib, bad = L.lib, L.AICP_ERR_INVALID
    c, keep = L.make_cloud(raws[0], np.asarray(poses[0], np.float64)[:3, 3])
    pz = np.ascontiguousarray(np.asarray(poses[0], F32).reshape(4, 4).T.reshape(16))
    T = np.full(16, 9.0, F32)
    res = (L.LocalizationResult if stream == "prior" else L.BuiltMapResult)()
    kept = C.c_uint32(9)

    def process(cloud=c, pose=pz, out_T=T, out=res):
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        return lib.aicp_hip_map_session_process(ctx.h, s.h, ref(cloud), None if pose is None else L._fptr(pose),
                                                None if out_T is None else L._fptr(out_T), ref(out), C.byref(kept))

    def untouched():
        assert len(m) == len(mp) and (T == 9.0).all() and res.status == 0 and res.map_points == 0 and kept.value == 9

    # before start
    assert process() == bad and "before start" in ctx.last_error()
    assert lib.aicp_hip_map_session_state(ctx.h, s.h, None, None, None, None) == bad
    assert lib.aicp_hip_map_session_start(ctx.h, s.h, None) == bad
    untouched()
    s.start()
    assert lib.aicp_hip_map_session_state(ctx.h, s.h, None, None, None, None) == 0  # every output is nullable
    assert lib.aicp_hip_map_session_last_timing(s.h, None, None) == 0
    for kw in (dict(cloud=None), dict(pose=None), dict(out_T=None), dict(out=None)):
        assert process(**kw) == bad, kw
    empty = L.Cloud()
    assert process(cloud=empty) == bad and "invalid reading" in ctx.last_error()
    assert lib.aicp_hip_map_session_process_accum(ctx.h, s.h, None, L._fptr(pz), L._fptr(T), C.byref(res),
                                                  C.byref(kept)) == bad
    untouched()
    st = s.state()
    assert st["n_processed"] == 0 and not st["ended"]
    # kept is nullable; the timing is of a call that registered
    assert lib.aicp_hip_map_session_process(ctx.h, s.h, C.byref(c), L._fptr(pz), L._fptr(T), C.byref(res), None) == 0
    assert res.status == 0 and res.map_points == len(mp) and not (T == 9.0).all()
    tm = s.last_timing()
    assert 0 < tm["device_ms"] <= tm["wall_ms"]
    s.close()
    m.free()
