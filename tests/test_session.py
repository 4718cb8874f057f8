"""The live App session on the device (aicp_hip_session_*, aicp_mapping_amd/session.py:
AppSession): App::processCloud one reading per call, with the reference, initialT_ and the count
resident in HBM between calls.

Checked against the oracle's replay of App (oracle.sequence: decisions, references, key counts,
ratio and iterations exact; 1e-6 rad / 1e-5 m; origins 1e-9), against the stream entry points over
the whole recording, and bit for bit against tests/session_reference.py, the same policy restated
as a host loop over the public one-pair calls (tests/test_session_cpu.py pins that loop to the
oracle). Every session run and every reference is computed once per module and shared."""
import functools

import numpy as np
import pytest

import accumulator_reference as ar
import raw_stream_reference as rs
import session_reference as sr
from aicp_mapping_amd import synthetic as sy
from test_sequence import _compare  # the stream tests' comparison with the oracle, unchanged

pytestmark = pytest.mark.gpu
RES = float(np.float32(0.2))
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def params(L, mode, freq, max_corr=1.0):
    return L.default_sequence_params(reference_update_frequency=freq, max_correction_magnitude=max_corr,
                                     flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if mode == "debug" else 0))


def strip(res):
    return {k: v for k, v in res.items() if k != "rc"}


def feed(ctx, L, st, mode, freq, raw, max_corr=1.0, cfg=None, between=None, session=None):
    """The readings of `st` through one session, one by one. Returns dict(T, out, kept, states,
    refs): per reading the correction, the result, the kept count, state() and reference() after
    the call."""
    from aicp_mapping_amd.session import AppSession

    s = session or AppSession(ctx, cfg=cfg, params=params(L, mode, freq, max_corr), prefilter=True if raw else None)
    s.start(st.first, st.first_origin)
    run = dict(T=[], out=[], kept=[], states=[], refs=[])
    for i, (r, o) in enumerate(zip(st.readings, st.origins)):
        if between:
            between(i)
        T, res, kept = s.process(r, o)
        run["T"].append(T)
        run["out"].append(strip(res))
        run["kept"].append(kept)
        run["states"].append(s.state())
        run["refs"].append(s.reference())
    if session is None:
        s.close()
    return run


def same_run(a, b):
    assert len(a["T"]) == len(b["T"])
    for i in range(len(a["T"])):
        assert same_bits(a["T"][i], b["T"][i]), i
        assert a["out"][i] == b["out"][i], i
        assert a["kept"][i] == b["kept"][i], i


# ---- test 1's fixture: 9 raw readings, reading 3 carries a 0.8 m jump -------------------------------
@functools.lru_cache(maxsize=None)
def raw_stream():
    return sy.make_stream(n_readings=9, n_points=20000, seed=8, half=12.0, jumps={3: (0, -0.8, 0)})


_SOLO = {}


def solo(ctx, L, mode, freq):
    """The raw fixture through a session of its own (computed once; with the cache statistics)."""
    key = (mode, freq)
    if key not in _SOLO:
        s0 = ctx.reference_cache_stats()
        run = feed(ctx, L, raw_stream(), mode, freq, raw=True, max_corr=0.4)
        s1 = ctx.reference_cache_stats()
        run["cache"] = {k: s1[k] - s0[k] for k in s0}
        _SOLO[key] = run
    return _SOLO[key]


_ORACLE = {}


def oracle_stream(oracle, mode, freq):
    key = (mode, freq)
    if key not in _ORACLE:
        st = raw_stream()
        _ORACLE[key] = oracle.sequence(st.first, st.first_origin, st.readings, st.origins,
                                       reference_update_frequency=freq, max_correction_magnitude=0.4, resolution=RES,
                                       working_mode=mode, prefilter_with=True)
    return _ORACLE[key]


@pytest.mark.parametrize("mode,freq", [("robot", 5), ("debug", 5), ("robot", 3)])
def test_raw_stream_reading_by_reading(ctx, oracle, L, mode, freq):
    """Feeding the recording one reading at a time gives App's replay (the oracle), the whole-
    recording entry point (debug mode, the same one-pair composition: every bit; robot mode, the
    windowed batches: the oracle's tolerances) and the host loop over one-pair calls (every bit); the
    reference's trees are built once per distinct reference."""
    st = raw_stream()
    run = solo(ctx, L, mode, freq)
    ref = oracle_stream(oracle, mode, freq)
    assert [r["accepted"] for r in ref] == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    promoted = [i for i, r in enumerate(ref) if r["is_reference"]]
    assert promoted == ([5] if freq == 5 else [2, 6])
    if freq == 5:
        assert [r["reference"] for r in ref] == [-1] * 6 + [5] * 3
    T = np.stack(run["T"])
    _compare(run["out"], ref, T)
    assert run["kept"] == [r["n_kept"] for r in ref]
    # state() follows: the reference id, the count of calls
    assert [s["reference"] for s in run["states"]] == [max([-1] + [p for p in promoted if p <= i]) for i in range(9)]
    assert [s["n_processed"] for s in run["states"]] == list(range(1, 10)) and not run["states"][-1]["ended"]
    # one tree build per distinct reference, every other reading reuses the resident trees
    n_refs = len({o["reference"] for o in run["out"]})
    assert run["cache"]["tree_builds"] == n_refs and run["cache"]["tree_hits"] == 9 - n_refs
    assert run["cache"]["ovl_builds"] == n_refs and run["cache"]["ovl_hits"] == 9 - n_refs
    # the whole recording in one call
    Tw, outw, done, rc = ctx.sequence_run(st.first, st.first_origin, st.readings, st.origins,
                                          params=params(L, mode, freq, 0.4), prefilter=True)
    assert rc == 0 and done == 9
    if mode == "debug":
        for i in range(9):
            assert same_bits(T[i], Tw[i]), i
            assert run["out"][i] == outw[i], i
    else:
        bits = all(same_bits(T[i], Tw[i]) for i in range(9))
        print(f"robot mode, frequency {freq}: session == windowed stream bit for bit: {bits}")
        for i, (a, b) in enumerate(zip(run["out"], outw)):
            for k in ("status", "accepted", "reference", "is_reference"):
                assert a[k] == b[k], (i, k)
            assert a["icp"]["overlap_keys"] == b["icp"]["overlap_keys"], i
            assert a["icp"]["iterations"] == b["icp"]["iterations"], i
            rr, tt = sy.rot_err(Tw[i], T[i])
            assert rr < 1e-6 and tt < 1e-5, (i, rr, tt)
            if a["accepted"]:
                np.testing.assert_allclose(a["corrected_origin"], b["corrected_origin"], rtol=0, atol=1e-9)
        # the host loop over one-pair calls: the same composition, every bit
        loop, _ = sr.replay(sr.CtxBackend(ctx, L, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                            st.origins, freq=freq, max_corr=0.4, debug=False, raw=True)
        for i, rec in enumerate(loop):
            assert same_bits(T[i], rec["T"]), i
            assert run["out"][i]["icp"] == rec["icp"], i
            assert (run["out"][i]["accepted"], run["out"][i]["is_reference"], run["out"][i]["reference"]) == \
                (rec["accepted"], rec["is_reference"], rec["reference"]), i


# ---- test 2: promotion edges, pre-filtered entry ---------------------------------------------------
@pytest.mark.parametrize("mode", ["robot", "debug"])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 4097])
def test_promotion_edges_prefiltered_entry(ctx, oracle, L, n, mode):
    """Every reading becomes the reference (frequency 1): after each call the session's reference is
    ctx.transform(T_i, reading i as registered) bit for bit, with corrected_origin as its origin."""
    from aicp_mapping_amd.session import AppSession

    st = sy.make_stream(n_readings=4, n_points=n, seed=7, half=18.0)
    loop, _ = sr.replay(sr.CtxBackend(ctx, L, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                        st.origins, freq=1, debug=mode == "debug", raw=False)
    assert [(r["status"], r["accepted"], r["is_reference"]) for r in loop] == [(0, 1, 1)] * 4
    s = AppSession(ctx, params=params(L, mode, 1))
    s.start(st.first, st.first_origin)
    pts, org = s.reference()
    assert same_bits(pts, st.first) and np.array_equal(org, st.first_origin)
    assert s.state()["reference"] == -1 and s.state()["n_processed"] == 0 and s.state()["reference_points"] == n
    for i, rec in enumerate(loop):
        T, res, kept = s.process(st.readings[i], st.origins[i])
        assert res["rc"] == 0 and res["status"] == 0 and res["accepted"] == 1 and res["is_reference"] == 1
        assert res["reference"] == i - 1 and kept == n
        assert same_bits(T, rec["T"]), i
        assert strip(res)["icp"] == rec["icp"], i
        pts, org = s.reference()
        assert same_bits(pts, ctx.transform(T, rec["registered"])), i
        assert np.array_equal(org, res["corrected_origin"])
        np.testing.assert_allclose(org, oracle.corrected_origin(T, rec["prior_origin"]), rtol=0, atol=1e-9)
        state = s.state()
        assert state["reference"] == i and state["n_processed"] == i + 1 and state["reference_points"] == n
        assert not state["ended"]
    assert (mode == "debug") == (not np.array_equal(loop[1]["registered"], st.readings[1]))
    s.close()


# ---- test 3: readings from the sweep accumulator -----------------------------------------------------
def scene_sweeps(k):
    """Reading k of the accumulator tests: 3 sweeps of ar.bridge_sweeps()'s scene (k = 0: those very
    sweeps), each in its own sensor frame, from poses a little further along."""
    if k == 0:
        return ar.bridge_sweeps()
    scene = sy.make_scene(7)
    sweeps, poses = [], []
    for i, (yaw, x) in enumerate([(3.0, -0.6), (-5.0, 0.0), (8.0, 0.7)]):
        x = x + 0.1 * k
        P = sy.make_T(yaw + k, 0.5 * i, -0.4 * i, (x, 0.1 * i + 0.03 * k, 0.7))
        world = sy.sample_scene(scene, np.random.default_rng(100 * k + 8 + i), (x, 0.0, 0.7), half=3.0, spacing=0.05)
        sweeps.append(sy.transform(np.linalg.inv(P), world))
        poses.append(P)
    return sweeps, poses


def fill(acc, k):
    sweeps, poses = scene_sweeps(k)
    for sw, P in zip(sweeps, poses):
        acc.push(sw, P)
    return poses[1][:3, 3].copy()


@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_readings_from_the_accumulator(ctx, L, mode):
    """process(acc) reads the accumulator's cloud where it lies: the same bits as process(getCloud())
    on a twin session, the accumulator unchanged, and free to be cleared and refilled at once."""
    from aicp_mapping_amd.accumulator import SweepAccumulator
    from aicp_mapping_amd.session import AppSession

    cap = max(sum(len(s) for s in scene_sweeps(k)[0]) for k in range(4))
    acc = SweepAccumulator(ctx, cap, batch_size=3)
    a = AppSession(ctx, params=params(L, mode, 5), prefilter=True)
    b = AppSession(ctx, params=params(L, mode, 5), prefilter=True)
    o0 = fill(acc, 0)
    first = acc.getCloud()
    a.start(acc, o0)
    b.start(first, o0)
    (pa, oa), (pb, ob) = a.reference(), b.reference()
    assert len(pa) >= 50 and same_bits(pa, pb) and np.array_equal(oa, ob) and np.array_equal(oa, o0)
    assert same_bits(acc.getCloud(), first)
    for k in (1, 2, 3):
        acc.clear()
        o = fill(acc, k)
        cloud = acc.getCloud()
        Ta, ra, ka = a.process(acc, o)
        assert same_bits(acc.getCloud(), cloud)  # left as it is
        acc.clear()
        fill(acc, (k + 1) % 4)  # the node's next reading starts at once
        Tb, rb, kb = b.process(cloud, o)
        assert same_bits(Ta, Tb) and ra == rb and ka == kb, k
        assert ra["status"] == 0 and ra["accepted"] == 1 and 50 <= ka < len(cloud)
        assert not np.array_equal(Ta, np.eye(4, dtype=F32))
        sa, sb = a.state(), b.state()
        assert same_bits(sa["initial_T"], sb["initial_T"]) and sa["n_processed"] == sb["n_processed"] == k
        # (debug mode from reading 2 on: the raw cloud is moved by a non-identity initialT_ first)
        assert not np.array_equal(sa["initial_T"], np.eye(4, dtype=F32))
    for s in (a, b):
        s.close()
    acc.free()


# ---- test 4: interleaving ----------------------------------------------------------------------------
def test_other_calls_between_readings_change_nothing(ctx, L):
    """An unrelated registration (which takes the context's reference cache) and a pre-filter between
    the process calls: the session rebuilds what it needs, no bit of its results changes."""
    other = sy.make_pair(3000, 3000, seed=5)
    cloud = raw_stream().readings[4]

    def between(i):
        if i % 2 == 1:
            ctx.register(other.ref, other.read)
        ctx.prefilter(cloud)

    s0 = ctx.reference_cache_stats()
    run = feed(ctx, L, raw_stream(), "robot", 5, raw=True, max_corr=0.4, between=between)
    s1 = ctx.reference_cache_stats()
    same_run(run, solo(ctx, L, "robot", 5))
    # the session noticed: 4 registrations took the cache, so 4 more builds than its 2 references
    assert s1["tree_builds"] - s0["tree_builds"] == 2 + 4 + 4


def test_reference_cache_off_changes_nothing(ctx, L):
    """aicp_hip_options::reference_cache = 0: nothing stays resident, every reading rebuilds the
    reference's trees and voxel map, and no bit of the results changes."""
    st = sy.make_stream(n_readings=4, n_points=4097, seed=7, half=18.0)
    s0 = ctx.reference_cache_stats()
    on = feed(ctx, L, st, "debug", 2, raw=False)
    s1 = ctx.reference_cache_stats()
    with ctx.options(reference_cache=0):
        off = feed(ctx, L, st, "debug", 2, raw=False)
    s2 = ctx.reference_cache_stats()
    same_run(on, off)
    assert [o["is_reference"] for o in on["out"]] == [0, 1, 0, 1]
    assert s1["tree_hits"] - s0["tree_hits"] == 2 and s2["tree_hits"] == s1["tree_hits"]
    assert s2["ovl_hits"] == s1["ovl_hits"]
    for a, b in zip(on["refs"], off["refs"]):
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_sessions_on_one_context(ctx, L):
    """Two sessions fed alternately each equal their solo run (the resident reference belongs to
    whichever registered last; the other rebuilds)."""
    from aicp_mapping_amd.session import AppSession

    st = raw_stream()
    x = AppSession(ctx, params=params(L, "robot", 5, 0.4), prefilter=True)
    y = AppSession(ctx, params=params(L, "debug", 5, 0.4), prefilter=True)
    x.start(st.first, st.first_origin)
    y.start(st.first, st.first_origin)
    rx, ry = dict(T=[], out=[], kept=[]), dict(T=[], out=[], kept=[])
    for i in range(9):
        for s, run in ((x, rx), (y, ry)):
            T, res, kept = s.process(st.readings[i], st.origins[i])
            run["T"].append(T)
            run["out"].append(strip(res))
            run["kept"].append(kept)
    same_run(rx, solo(ctx, L, "robot", 5))
    same_run(ry, solo(ctx, L, "debug", 5))
    x.close()
    y.close()


# ---- test 5: endings -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_emptied_reading_ends_the_session_and_start_revives_it(ctx, L, mode):
    from aicp_mapping_amd.session import AppSession

    st = sy.make_stream(n_readings=5, n_points=20000, seed=3, half=12.0)
    s = AppSession(ctx, params=params(L, mode, 5), prefilter=True)
    s.start(st.first, st.first_origin)
    first3 = [s.process(st.readings[i], st.origins[i]) for i in range(3)]
    assert all(r[1]["status"] == 0 for r in first3)
    before = s.state()
    T, res, kept = s.process(rs.scattered(), st.origins[3], raise_on_error=False)
    assert res["rc"] == L.AICP_ERR_INVALID and res["status"] == L.AICP_ERR_INVALID and res["icp"]["status"] == L.AICP_ERR_INVALID
    assert kept == 0 and not res["accepted"] and res["reference"] == -1 and np.array_equal(T, np.eye(4, dtype=F32))
    after = s.state()
    assert after["ended"] and after["n_processed"] == 4 and after["reference"] == before["reference"]
    assert same_bits(after["initial_T"], before["initial_T"])
    with pytest.raises(L.AicpError) as e:
        s.process(st.readings[4], st.origins[4])
    assert e.value.code == L.AICP_ERR_INVALID and "ended at reading 3" in str(e.value)
    assert s.state()["n_processed"] == 4
    s.start(st.first, st.first_origin)  # revives it, from the beginning
    state = s.state()
    assert not state["ended"] and state["n_processed"] == 0 and state["reference"] == -1
    assert np.array_equal(state["initial_T"], np.eye(4, dtype=F32))
    again = s.process(st.readings[0], st.origins[0])
    assert same_bits(again[0], first3[0][0]) and again[1] == first3[0][1] and again[2] == first3[0][2]
    s.close()


def test_registration_error_ends_the_session(ctx, L):
    """test_sequence_error_ends_stream's case: reading 6, 200 m away with a 5 m matcher radius."""
    from aicp_mapping_amd.session import AppSession

    st = sy.make_stream(n_readings=9, n_points=4000, seed=9, half=15.0)
    st.readings[6] = (st.readings[6] + F32(200.0)).astype(F32)
    st.origins[6] = st.origins[6] + 200.0
    cfg = L.default_config(nn_max_dist=5.0)
    Tw, outw, done, rcw = ctx.sequence_run(st.first, st.first_origin, st.readings, st.origins, cfg=cfg,
                                           raise_on_error=False)
    assert rcw == L.AICP_ERR_CONVERGENCE and done == 7
    s = AppSession(ctx, cfg=cfg, params=params(L, "robot", 5))
    s.start(st.first, st.first_origin)
    for i in range(6):
        T, res, kept = s.process(st.readings[i], st.origins[i])
        assert res["status"] == 0 and res["reference"] == outw[i]["reference"]
    before = s.state()
    pts_before, _ = s.reference()
    T, res, kept = s.process(st.readings[6], st.origins[6], raise_on_error=False)
    assert res["rc"] == L.AICP_ERR_CONVERGENCE and res["status"] == L.AICP_ERR_CONVERGENCE and not res["accepted"]
    assert res["reference"] == 4
    after = s.state()
    assert after["ended"] and after["n_processed"] == 7 and after["reference"] == before["reference"] == 4
    assert same_bits(after["initial_T"], before["initial_T"]) and same_bits(s.reference()[0], pts_before)
    with pytest.raises(L.AicpError) as e:
        s.process(st.readings[7], st.origins[7])
    assert e.value.code == L.AICP_ERR_INVALID
    with pytest.raises(L.ConvergenceError):
        s.start(st.first, st.first_origin)
        s.process(st.readings[6], st.origins[6])
    s.close()


@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_dropped_reading_leaves_the_state(ctx, L, mode):
    """Reading 3 of the raw fixture is dropped: state() and reference() are what they were, except
    n_processed, initialT_ included."""
    run = solo(ctx, L, mode, 5)
    assert run["out"][2]["accepted"] and not run["out"][3]["accepted"] and run["out"][3]["status"] == 0
    a, b = run["states"][2], run["states"][3]
    assert (b["n_processed"], a["n_processed"]) == (4, 3)
    assert a["reference"] == b["reference"] and a["reference_points"] == b["reference_points"] and not b["ended"]
    assert same_bits(a["initial_T"], b["initial_T"]) and not np.array_equal(a["initial_T"], np.eye(4, dtype=F32))
    assert same_bits(run["refs"][2][0], run["refs"][3][0]) and np.array_equal(run["refs"][2][1], run["refs"][3][1])
    assert run["out"][3]["corrected_origin"] == [0.0, 0.0, 0.0] and not run["out"][3]["is_reference"]
    # the accepted reading after it moves initialT_ again
    assert not same_bits(run["states"][4]["initial_T"], b["initial_T"])


def test_invalid_arguments(ctx, L):
    import ctypes as C

    from aicp_mapping_amd.session import AppSession

    st = sy.make_stream(n_readings=1, n_points=1024, seed=7, half=18.0)
    for bad in (dict(reference_update_frequency=0), dict(flags=64), dict(flags=L.AICP_RUN_OVERLAP, resolution=0.0),
                dict(max_correction_magnitude=float("nan"))):
        with pytest.raises(L.AicpError) as e:
            AppSession(ctx, params=L.default_sequence_params(**bad))
        assert e.value.code == L.AICP_ERR_INVALID
    with pytest.raises(L.AicpError):
        AppSession(ctx, prefilter=L.default_prefilter(normal_k=25))
    s = AppSession(ctx)
    for call in (lambda: s.process(st.readings[0], st.origins[0]), s.state, s.reference):
        with pytest.raises(L.AicpError) as e:  # before start
            call()
        assert e.value.code == L.AICP_ERR_INVALID
    with pytest.raises(L.AicpError) as e:
        s.start(np.zeros((0, 3), F32))
    assert e.value.code == L.AICP_ERR_INVALID
    s.start(st.first, st.first_origin)
    with pytest.raises(L.AicpError) as e:  # an invalid cloud is refused; it is not a reading
        s.process(np.zeros((0, 3), F32))
    assert e.value.code == L.AICP_ERR_INVALID
    state = s.state()
    assert not state["ended"] and state["n_processed"] == 0
    T, res = np.zeros(16, F32), L.SequenceResult()
    c, keep = L.make_cloud(st.readings[0], st.origins[0])
    lib = L.lib
    assert lib.aicp_hip_session_process(ctx.h, s.h, None, L._fptr(T), C.byref(res), None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_process(ctx.h, s.h, C.byref(c), None, C.byref(res), None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_process(ctx.h, s.h, C.byref(c), L._fptr(T), None, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_process(ctx.h, None, C.byref(c), L._fptr(T), C.byref(res), None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_process_accum(ctx.h, s.h, None, None, L._fptr(T), C.byref(res), None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_start(ctx.h, s.h, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_start_accum(ctx.h, s.h, None, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_create(ctx.h, None, None, None, C.byref(C.c_void_p())) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_process(ctx.h, s.h, C.byref(c), L._fptr(T), C.byref(res), None) == L.AICP_OK
    assert s.state()["n_processed"] == 1
    s.close()


# ---- test 6: a point-to-point chain --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_point_to_point_chain(ctx, oracle, L, mode):
    """PointToPointErrorMinimizer (knn_normals = 0) runs in the session, as the one-pair calls serve
    it; the whole-recording stream keeps refusing it."""
    from aicp_mapping_amd.session import AppSession

    cfg = L.default_config(point_to_point=True)
    assert cfg.knn_normals == 0
    st = sy.make_stream(n_readings=4, n_points=4097, seed=7, half=18.0)
    loop, _ = sr.replay(sr.CtxBackend(ctx, L, cfg=cfg, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                        st.origins, freq=1, debug=mode == "debug", raw=False)
    assert all(r["status"] == 0 and r["iterations"] > 0 for r in loop)
    run = feed(ctx, L, st, mode, 1, raw=False, cfg=cfg)
    for i, rec in enumerate(loop):
        assert same_bits(run["T"][i], rec["T"]), i
        assert run["out"][i]["icp"] == rec["icp"], i
        assert (run["out"][i]["accepted"], run["out"][i]["is_reference"], run["out"][i]["reference"]) == \
            (rec["accepted"], rec["is_reference"], rec["reference"]), i
        if rec["is_reference"]:
            assert same_bits(run["refs"][i][0], ctx.transform(rec["T"], rec["registered"])), i
    _, _, _, rc = ctx.sequence_run(st.first, st.first_origin, st.readings, st.origins, cfg=cfg, raise_on_error=False)
    assert rc == L.AICP_ERR_UNSUPPORTED
