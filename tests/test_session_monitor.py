"""The quality monitor per reading in the live sessions (aicp_hip_session_set_monitor and its map
twin; AppSession / MapSession monitor=, set_monitor, last_monitor, monitor_counters) and its
resident core through aicp_hip_test_monitor_resident.

Every result is compared as bytes(aicp_monitor_result) (56 bytes) with what the stand-alone
ctx.monitor gives for the clouds a caller could have composed by hand: the reference downloaded
before the call (or the map crop taken before it), the reading as it was registered, and the
correction the call returned. One case goes against tests/monitor_reference.py on the CPU oracle, so
that the chain is not checked against itself only. A session with the monitor on returns what a
session without it returns, bit for bit. Session runs and replays are computed once per module."""
import numpy as np
import pytest

import monitor_reference as mr
import raw_stream_reference as rs
import session_reference as sr
from aicp_mapping_amd import synthetic as sy
from test_map_session import assert_same_run, feed as map_feed
from test_monitor import assert_matches
from test_raw_stream import make_map, params as map_params
from test_session import RES, params, raw_stream, same_bits, same_run, solo, strip
from test_session_risk import new_session as new_risk_session, stream as risk_stream

pytestmark = pytest.mark.gpu
F32 = np.float32
ZERO = bytes(56)


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def chain(L, ratio=None, **kw):
    c = L.default_config(**kw)
    if ratio is not None:
        c.trimmed_ratio = ratio
    return c


# ---- 1. the resident core on guarded buffers ----------------------------------------------------
# readings: one point; one NN chunk and both sides of it; both sides of a 256-thread block of
# k_mon_stage and of a reduction slab; several blocks. references: one point, a bucket and one more,
# a few leaves, both sides of a 4096-value reduction chunk
EDGES = [(1, 1), (9, 2), (300, 63), (300, 64), (300, 65), (9, 255), (4097, 256), (300, 257), (4097, 1025)]
T_RIGID = sy.make_T(yaw_deg=7.0, pitch_deg=-2.0, roll_deg=1.5, t=(0.31, -0.22, 0.13)).astype(F32)


def clouds(n_ref, n_read):
    rng = np.random.default_rng(1000 * n_ref + n_read)
    ref = (rng.random((n_ref, 3)) * 4).astype(F32)
    read = (rng.random((n_read, 3)) * 4).astype(F32)
    return ref, read


@pytest.mark.parametrize("ident", [False, True], ids=["rigid", "identity"])
@pytest.mark.parametrize("n_ref,n_read", EDGES)
def test_resident_core_equals_the_uploaded_monitor(ctx, n_ref, n_read, ident):
    """Two runs in a row on one reference tree (built, then reused): the second run's bytes are
    ctx.monitor's, no guard word changed and no input changed."""
    ref, read = clouds(n_ref, n_read)
    T = np.eye(4, dtype=F32) if ident else T_RIGID
    want = ctx.monitor(ref, read, T)
    one, dirty1, c1 = ctx.test_monitor_resident(ref, read, T, runs=1)
    two, dirty2, c2 = ctx.test_monitor_resident(ref, read, T, runs=2)
    assert one["bytes"] == want["bytes"] and two["bytes"] == want["bytes"]
    assert dirty1 == 0 and dirty2 == 0
    assert c1 == dict(readings=1, trees=2, reference_reuses=0, chain_trees=0)
    assert c2 == dict(readings=2, trees=3, reference_reuses=1, chain_trees=0)


@pytest.mark.parametrize("kw,chain_trees", [(dict(nn_epsilon=3.16), 0),
                                            (dict(nn_epsilon=0.0, nn_max_dist=float("inf"), bucket_size=8), 0),
                                            (dict(nn_epsilon=3.16, bucket_size=4), 1)],
                         ids=["eps3.16", "eps0-bucket8", "bucket4"])
def test_resident_core_paired_mean(ctx, L, kw, chain_trees):
    """The chain matcher's search: its own launch, direction 0's when it is the same search, and in
    a second reference tree (built once for both runs) at another bucket size."""
    ref, read = clouds(4097, 1025)
    read = (ref[:1025] + F32(0.01) * read).astype(F32)  # (pairs within the matcher's reach)
    cfg = chain(L, ratio=0.7, **kw)
    want = ctx.monitor(ref, read, T_RIGID, cfg=cfg)
    got, dirty, cnt = ctx.test_monitor_resident(ref, read, T_RIGID, cfg=cfg, runs=2)
    assert got["bytes"] == want["bytes"] and dirty == 0 and got["paired_kept"] > 0
    assert cnt == dict(readings=2, trees=3, reference_reuses=1, chain_trees=chain_trees)


# ---- 2. AppSession on the raw fixture -------------------------------------------------------------
_MON = {}


def feed_monitored(ctx, L, st, mode, freq, raw, max_corr, monitor=True, cfg=None, switch=None, between=None,
                   session=None):
    """feed() of tests/test_session.py with the monitor: per reading also the reference before the
    call, last_monitor() after it and the counters at the end. switch: reading -> monitor argument
    set before that reading."""
    from aicp_mapping_amd.session import AppSession

    s = session or AppSession(ctx, cfg=cfg, params=params(L, mode, freq, max_corr), prefilter=True if raw else None,
                              monitor=monitor)
    s.start(st.first, st.first_origin)
    run = dict(T=[], out=[], kept=[], states=[], refs=[], before=[], mon=[], initT=[])
    assert s.last_monitor()["valid"] is False and s.last_monitor()["bytes"] == ZERO
    for i, (r, o) in enumerate(zip(st.readings, st.origins)):
        if switch and i in switch:
            s.set_monitor(switch[i])
        if between:
            between(i)
        run["before"].append(s.reference()[0])
        run["initT"].append(s.state()["initial_T"])
        T, res, kept = s.process(r, o)
        run["T"].append(T)
        run["out"].append(strip(res))
        run["kept"].append(kept)
        run["states"].append(s.state())
        run["refs"].append(s.reference())
        run["mon"].append(s.last_monitor())
    run["counters"] = s.monitor_counters()
    if session is None:
        s.close()
    return run


def monitored(ctx, L, mode, freq):
    if (mode, freq) not in _MON:
        _MON[(mode, freq)] = feed_monitored(ctx, L, raw_stream(), mode, freq, True, 0.4)
    return _MON[(mode, freq)]


def same_states(a, b):
    for i, (x, y) in enumerate(zip(a["states"], b["states"])):
        assert {k: v for k, v in x.items() if k != "initial_T"} == {k: v for k, v in y.items() if k != "initial_T"}, i
        assert same_bits(x["initial_T"], y["initial_T"]), i
    for i, (x, y) in enumerate(zip(a["refs"], b["refs"])):
        assert same_bits(x[0], y[0]) and np.array_equal(x[1], y[1]), i


@pytest.mark.parametrize("mode,freq", [("robot", 5), ("debug", 5), ("robot", 3)])
def test_app_session_reading_by_reading(ctx, oracle, L, mode, freq):
    st = raw_stream()
    run = monitored(ctx, L, mode, freq)
    loop, _ = sr.replay(sr.CtxBackend(ctx, L, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                        st.origins, freq=freq, max_corr=0.4, debug=mode == "debug", raw=True)
    for i, rec in enumerate(loop):
        got = run["mon"][i]
        assert got["valid"], i
        want = ctx.monitor(run["before"][i], rec["registered"], run["T"][i])
        assert got["bytes"] == want["bytes"], (i, got, want)
    # reading 3 is dropped: its monitor is valid all the same, and the state stays
    assert [o["accepted"] for o in run["out"]] == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert same_bits(run["refs"][3][0], run["refs"][2][0]) and same_bits(run["states"][3]["initial_T"],
                                                                         run["states"][2]["initial_T"])
    # a promoted reading was measured against the old reference (`before`), which the call replaced
    promoted = [i for i, o in enumerate(run["out"]) if o["is_reference"]]
    assert promoted == ([5] if freq == 5 else [2, 6])
    for i in promoted:
        assert not same_bits(run["before"][i], run["refs"][i][0])
    # the monitor changes nothing the session returns or keeps
    plain = solo(ctx, L, mode, freq)
    same_run(run, plain)
    same_states(run, plain)
    n_refs = len({o["reference"] for o in run["out"]})
    assert run["counters"] == dict(readings=9, trees=9 + n_refs, reference_reuses=9 - n_refs, chain_trees=0)


# ---- 3. promotion edges, pre-filtered entry ---------------------------------------------------------
@pytest.mark.parametrize("freq", [1, 100])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 4097])
def test_promotion_edges(ctx, L, n, freq):
    """Frequency 1: every reading is promoted, so every reading rebuilds the reference tree (and
    reading i + 1 is measured against T_i * reading i). Frequency 100: one tree serves them all."""
    st = sy.make_stream(n_readings=4, n_points=n, seed=7, half=18.0)
    st.first, st.first_origin = sy.stream_first(7, 3001, half=18.0)
    run = feed_monitored(ctx, L, st, "robot", freq, False, 1.0)
    for i in range(4):
        assert run["mon"][i]["valid"] and run["out"][i]["is_reference"] == (1 if freq == 1 else 0), i
        want = ctx.monitor(run["before"][i], st.readings[i], run["T"][i])
        assert run["mon"][i]["bytes"] == want["bytes"], i
        if i and freq == 1:
            assert same_bits(run["before"][i], ctx.transform(run["T"][i - 1], st.readings[i - 1]))
    assert len(run["before"][0]) == 3001
    if freq == 1:
        assert run["counters"] == dict(readings=4, trees=8, reference_reuses=0, chain_trees=0)
    else:
        assert run["counters"] == dict(readings=4, trees=5, reference_reuses=3, chain_trees=0)


# ---- 4. switching, other calls in between, two sessions ---------------------------------------------
def test_switching_the_monitor(ctx, L):
    on = monitored(ctx, L, "robot", 5)
    run = feed_monitored(ctx, L, raw_stream(), "robot", 5, True, 0.4, monitor=None,
                         switch={2: True, 6: None, 7: dict(quantile=0.6)})
    same_run(run, on)
    for i in range(9):
        if i in (0, 1, 6):
            assert not run["mon"][i]["valid"] and run["mon"][i]["bytes"] == ZERO, i
        else:
            assert run["mon"][i]["valid"] and run["mon"][i]["bytes"] == on["mon"][i]["bytes"], i
    assert run["counters"]["readings"] == 6


def test_a_standalone_monitor_between_readings_changes_nothing(ctx, L):
    """ctx.monitor on unrelated clouds (with a chain at another bucket size, so that all of the
    context's monitor buffers are rewritten) before every reading: the session's reference tree is
    its own."""
    on = monitored(ctx, L, "robot", 5)
    a, b = clouds(30000, 25000)
    cfg = chain(L, ratio=0.5, bucket_size=4)
    run = feed_monitored(ctx, L, raw_stream(), "robot", 5, True, 0.4, between=lambda i: ctx.monitor(a, b, cfg=cfg))
    same_run(run, on)
    assert [m["bytes"] for m in run["mon"]] == [m["bytes"] for m in on["mon"]]
    assert run["counters"] == on["counters"]


def test_two_monitored_sessions_on_one_context(ctx, L):
    from aicp_mapping_amd.session import AppSession

    on5, on3 = monitored(ctx, L, "robot", 5), monitored(ctx, L, "robot", 3)
    st = raw_stream()
    s5 = AppSession(ctx, params=params(L, "robot", 5, 0.4), prefilter=True, monitor=True)
    s3 = AppSession(ctx, params=params(L, "robot", 3, 0.4), prefilter=True, monitor=True)
    s5.start(st.first, st.first_origin)
    s3.start(st.first, st.first_origin)
    for i in range(9):
        for s, on in ((s5, on5), (s3, on3)):
            T, res, kept = s.process(st.readings[i], st.origins[i])
            assert same_bits(T, on["T"][i]) and strip(res) == on["out"][i], i
            assert s.last_monitor()["bytes"] == on["mon"][i]["bytes"], i
    assert s5.monitor_counters() == on5["counters"] and s3.monitor_counters() == on3["counters"]
    s5.close()
    s3.close()


# ---- 5. the paired mean through the session's chain ----------------------------------------------------
@pytest.mark.parametrize("kw,chain_trees", [(dict(), 0), (dict(nn_epsilon=0.0), 0), (dict(bucket_size=4), 1),
                                            (dict(point_to_point=True), 0)],
                         ids=["default", "eps0", "bucket4", "p2p"])
def test_paired_mean_through_the_sessions_chain(ctx, L, kw, chain_trees):
    """The chain is the session's, at the reading's own tuned ratio (the result's
    icp.trimmed_ratio). Pre-filtered entry, one reference for all readings."""
    st = sy.make_stream(n_readings=3, n_points=4097, seed=7, half=18.0)
    cfg = L.default_config(**kw)
    if "nn_epsilon" not in kw:
        assert abs(cfg.nn_epsilon - 3.16) < 1e-6
    run = feed_monitored(ctx, L, st, "robot", 100, False, 1.0, monitor=dict(paired=True), cfg=cfg)
    ratios = set()
    for i in range(3):
        c = L.default_config(**kw)
        c.trimmed_ratio = run["out"][i]["icp"]["trimmed_ratio"]
        ratios.add(c.trimmed_ratio)
        want = ctx.monitor(run["before"][i], st.readings[i], run["T"][i], cfg=c)
        got = run["mon"][i]
        assert got["valid"] and got["bytes"] == want["bytes"], (i, got, want)
        assert got["paired_kept"] > 0 and np.isfinite(got["paired_mean_dist"])
    plain = feed_monitored(ctx, L, st, "robot", 100, False, 1.0, monitor=None, cfg=L.default_config(**kw))
    same_run(run, plain)
    # (a bucket-4 chain keeps its second reference tree as it keeps the first)
    assert run["counters"] == dict(readings=3, trees=4, reference_reuses=2, chain_trees=chain_trees)


# ---- 6. the gated session ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(L):
    import svm_reference as svm

    m = L.SvmModel(svm.golden(svm.MODELS["opencv3"][0]))
    yield m
    m.close()


def feed_risk(ctx, L, model, thr, monitor):
    st, first_pose, poses = risk_stream()
    s = new_risk_session(ctx, L, model, thr, False)
    s.set_monitor(monitor)
    s.start(st.first, pose=first_pose)
    run = dict(T=[], out=[], kept=[], rec=[], before=[], mon=[], refs=[])
    for i in range(len(poses)):
        run["before"].append(s.reference()[0])
        T, res, kept, rec = s.process(st.readings[i], pose=poses[i])
        run["T"].append(T)
        run["out"].append(strip(res))
        run["kept"].append(kept)
        run["rec"].append(rec)
        run["mon"].append(s.last_monitor())
        run["refs"].append(s.reference()[0])
    run["counters"] = s.monitor_counters()
    s.close()
    return run


def test_gate_that_always_closes_leaves_no_result(ctx, L, golden):
    run = feed_risk(ctx, L, golden, 0.0, True)
    assert all(r["registered"] == 0 for r in run["rec"])
    assert all(not m["valid"] and m["bytes"] == ZERO for m in run["mon"])
    assert run["counters"] == dict(readings=0, trees=0, reference_reuses=0, chain_trees=0)
    same_run(run, feed_risk(ctx, L, golden, 0.0, None))


def test_gate_that_never_closes_monitors_every_reading(ctx, L, golden):
    st, _, poses = risk_stream()
    run = feed_risk(ctx, L, golden, 1.0, True)
    assert all(r["registered"] == 1 for r in run["rec"])
    for i in range(len(poses)):
        want = ctx.monitor(run["before"][i], ctx.prefilter(st.readings[i]), run["T"][i])
        assert run["mon"][i]["valid"] and run["mon"][i]["bytes"] == want["bytes"], i
    plain = feed_risk(ctx, L, golden, 1.0, None)
    same_run(run, plain)
    assert all(same_bits(a, b) for a, b in zip(run["refs"], plain["refs"]))
    n_refs = len({o["reference"] for o in run["out"]})
    n = len(poses)
    assert run["counters"] == dict(readings=n, trees=n + n_refs, reference_reuses=n - n_refs, chain_trees=0)


# ---- 7. the map sessions ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(oracle):
    return dict(prior=rs.prior_world(oracle), built=rs.built_world(oracle))


def map_feed_monitored(ctx, L, stream, world, debug):
    from aicp_mapping_amd.map_session import MapSession

    mp, raws, poses, _ = world
    prm = map_params(L, stream, debug)
    m = make_map(ctx, stream, mp)
    s = MapSession(ctx, m, params=prm, prefilter=True, monitor=True)
    s.start()
    out = dict(T=[], res=[], kept=[], rc=0, crops=[], regs=[], mon=[])
    for r, P in zip(raws, poses):
        out["crops"].append(m.crop(prm.crop_min, prm.crop_max, P))  # (the crop is taken at the pose as given)
        moved = ctx.transform(s.state()["initial_T"], r) if debug else r
        out["regs"].append(ctx.prefilter(moved))
        T, d, k = s.process(r, P, raise_on_error=False)
        out["rc"] = d.pop("rc")
        out["T"].append(T)
        out["res"].append(d)
        out["kept"].append(k)
        out["mon"].append(s.last_monitor())
    out["done"] = len(out["res"])
    out["T"] = np.array(out["T"], F32).reshape(-1, 4, 4)
    out["final"] = m.getCloud()
    out["counters"] = s.monitor_counters()
    s.close()
    m.free()
    return out


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
@pytest.mark.parametrize("stream", ["prior", "built"])
def test_map_session(ctx, L, worlds, stream, debug):
    """Per reading the monitor of (the crop taken just before the call at the call's pose, the
    reading as registered, T); debug mode registers the raw reading moved by initialT_ and then
    pre-filtered, against the crop at the pose as given (the streams' rule). The twin session without
    the monitor on a twin map returns the same and leaves the same map."""
    out = map_feed_monitored(ctx, L, stream, worlds[stream], debug)
    n = len(worlds[stream][1])
    assert out["rc"] == 0 and out["done"] == n
    for i in range(n):
        assert out["res"][i]["crop_points"] == len(out["crops"][i]), i
        assert out["kept"][i] == len(out["regs"][i]), i
        want = ctx.monitor(out["crops"][i], out["regs"][i], out["T"][i])
        assert out["mon"][i]["valid"] and out["mon"][i]["bytes"] == want["bytes"], i
    assert [r["accepted"] for r in out["res"]].count(0) >= 1  # (a dropped reading is monitored too)
    twin = map_feed(ctx, L, stream, *worlds[stream][:3], debug)
    assert_same_run(out, twin)
    assert out["counters"] == dict(readings=n, trees=2 * n, reference_reuses=0, chain_trees=0)


# ---- 8. endings and arguments --------------------------------------------------------------------------
def test_app_session_endings(ctx, L):
    from aicp_mapping_amd.session import AppSession

    st = raw_stream()
    errors = {}
    for monitor in (None, True):
        s = AppSession(ctx, params=params(L, "robot", 5, 0.4), prefilter=True, monitor=monitor)
        s.start(st.first, st.first_origin)
        s.process(st.readings[0], st.origins[0])
        assert s.last_monitor()["valid"] == (monitor is True)
        T, res, kept = s.process(rs.scattered(), st.origins[1], raise_on_error=False)  # the pre-filter empties it
        errors[monitor] = (res["rc"], strip(res), kept, ctx.last_error())
        assert res["rc"] == L.AICP_ERR_INVALID and s.state()["ended"]
        assert not s.last_monitor()["valid"] and s.last_monitor()["bytes"] == ZERO
        s.close()
    assert errors[None] == errors[True]
    # a failed registration: test_session.py's case, reading 6 is 200 m away with a 5 m matcher radius
    st = sy.make_stream(n_readings=8, n_points=4000, seed=9, half=15.0)
    st.readings[6] = (st.readings[6] + F32(200.0)).astype(F32)
    st.origins[6] = st.origins[6] + 200.0
    for monitor in (None, True):
        s = AppSession(ctx, cfg=L.default_config(nn_max_dist=5.0), params=params(L, "robot", 5), monitor=monitor)
        s.start(st.first, st.first_origin)
        for i in range(6):
            s.process(st.readings[i], st.origins[i])
        T, res, kept = s.process(st.readings[6], st.origins[6], raise_on_error=False)
        errors[monitor] = (res["rc"], strip(res), kept, ctx.last_error())
        assert res["rc"] == L.AICP_ERR_CONVERGENCE and s.state()["ended"]
        assert not s.last_monitor()["valid"] and s.last_monitor()["bytes"] == ZERO
        s.close()
    assert errors[None] == errors[True]


def test_map_session_endings(ctx, L, worlds):
    from aicp_mapping_amd.map_session import MapSession

    mp, raws, poses, _ = worlds["prior"]
    far = np.array(poses[1], np.float64)
    far[:3, 3] += 500.0  # no map point in the crop box
    for reading, pose, why in ((raws[1], far, "empty map crop"), (rs.scattered(), poses[1], "keeps no point")):
        errors = {}
        for monitor in (None, True):
            m = make_map(ctx, "prior", mp)
            s = MapSession(ctx, m, params=map_params(L, "prior", False), prefilter=True, monitor=monitor)
            s.start()
            s.process(raws[0], poses[0])
            assert s.last_monitor()["valid"] == (monitor is True)
            T, d, k = s.process(reading, pose, raise_on_error=False)
            errors[monitor] = (d, k, ctx.last_error())
            assert d["rc"] == L.AICP_ERR_INVALID and why in ctx.last_error() and s.state()["ended"]
            assert not s.last_monitor()["valid"] and s.last_monitor()["bytes"] == ZERO
            s.close()
            m.free()
        assert errors[None] == errors[True]


def test_a_monitor_error_costs_only_the_result(ctx, L):
    """The monitor's own errors, through the test entry (a registration does not survive such
    clouds): the reference of tests/tree_reference.py whose tree is deeper than the device stacks (48
    levels; tests/test_tree_kernels.py builds it) is refused as the stand-alone monitor refuses it,
    by a planned build (reported after the wait; k_mon_guard has kept the searches out of the tree)
    and by a polled one. The core runs again afterwards."""
    import tree_reference as tr

    deep = np.ascontiguousarray(tr.clouds_of(tr.OVER_LIMIT.data)[0][:, :3], F32)
    read = clouds(9, 300)[1]
    with pytest.raises(L.AicpError) as e:
        ctx.monitor(deep, read)
    want = e.value.code
    with pytest.raises(L.AicpError) as e:
        ctx.test_monitor_resident(deep, read, T_RIGID)
    assert e.value.code == want == L.AICP_ERR_UNSUPPORTED and "48 levels" in str(e.value)
    with pytest.raises(L.AicpError) as e:
        with ctx.options(tree_plan=-1):
            ctx.test_monitor_resident(deep, read, T_RIGID)
    assert e.value.code == L.AICP_ERR_UNSUPPORTED and "48 levels" in str(e.value)
    # the core runs again after an error
    ref, rd = clouds(300, 65)
    assert ctx.test_monitor_resident(ref, rd, T_RIGID)[0]["bytes"] == ctx.monitor(ref, rd, T_RIGID)["bytes"]


def test_arguments(ctx, L):
    import ctypes as C

    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.session import AppSession

    s = AppSession(ctx)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(L.AicpError) as e:
            s.set_monitor(dict(quantile=q))
        assert e.value.code == L.AICP_ERR_INVALID
    lib = L.lib
    prm, res, valid, cnt = L.default_monitor_params(), L.MonitorResult(), C.c_int32(), (C.c_uint64 * 4)()
    assert lib.aicp_hip_session_set_monitor(None, s.h, C.byref(prm)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_set_monitor(ctx.h, None, C.byref(prm)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_last_monitor(None, C.byref(res), C.byref(valid)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_last_monitor(s.h, None, C.byref(valid)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_last_monitor(s.h, C.byref(res), None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_monitor_counters(None, cnt) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_monitor_counters(s.h, None) == L.AICP_ERR_INVALID
    assert s.last_monitor()["valid"] is False and s.monitor_counters()["readings"] == 0  # before start
    s.close()
    m = make_map(ctx, "prior", clouds(300, 1)[0])
    ms = MapSession(ctx, m)
    with pytest.raises(L.AicpError):
        ms.set_monitor(dict(quantile=2.0))
    assert lib.aicp_hip_mapsession_set_monitor(ctx.h, None, C.byref(prm)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_mapsession_last_monitor(ms.h, None, C.byref(valid)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_mapsession_monitor_counters(ms.h, None) == L.AICP_ERR_INVALID
    assert ms.last_monitor()["bytes"] == ZERO
    ms.close()
    m.free()
    ref, rd = clouds(9, 2)
    T16 = np.eye(4, dtype=F32).reshape(16)
    assert lib.aicp_hip_test_monitor_resident(ctx.h, C.byref(prm), None, L._fptr(ref), 9, L._fptr(rd), 0, L._fptr(T16), 1,
                                              C.byref(res), C.byref(C.c_uint64()), cnt) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_test_monitor_resident(ctx.h, C.byref(prm), None, L._fptr(ref), 9, L._fptr(rd), 2, None, 1,
                                              C.byref(res), C.byref(C.c_uint64()), cnt) == L.AICP_ERR_INVALID


# ---- 9. against the restatement on the CPU oracle --------------------------------------------------------
def test_against_the_numpy_restatement(ctx, oracle, L):
    """Reading 1 of the raw fixture (robot mode) through the oracle's kNN, at the stand-alone
    monitor's own tolerances (tests/test_monitor.py: assert_matches)."""
    st = raw_stream()
    run = monitored(ctx, L, "robot", 5)
    got = run["mon"][1]
    want = mr.monitor(oracle, run["before"][1], ctx.prefilter(st.readings[1]), T=run["T"][1])
    assert_matches(got, want)
