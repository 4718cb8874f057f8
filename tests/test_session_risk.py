"""The live App session with failure_prediction_mode (aicp_hip_session_create_risk and the _pose /
_risk calls, AppSession(..., risk=...)): the risk gate served one reading per call on the session's
resident buffers, the gated branch taken on the device by k_session_gate_promote.

Every bar is exact: reading by reading the session gives aicp_hip_sequence_run_risk's bytes on the
whole recording (T, every aicp_sequence_result and aicp_pipeline_record field), and after every
call reference(), reference_pose() and initialT_ are those of the host loop of
tests/session_risk_reference.py. The stream fixture is tests/test_risk_pipeline.py's; the
placement of the gate (a test-written model with raw = overlap - X) is asserted on the host loop
before the device's session is looked at. Runs are computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import raw_stream_reference as rs
import risk_reference as rr
import session_risk_reference as srr
import svm_reference as sr
from aicp_mapping_amd import synthetic as sy
from test_alignment_risk import ORIGIN_A, ORIGIN_B, scene_cloud

pytestmark = pytest.mark.gpu

RES = float(np.float32(0.2))
VIEW = 270.0
F32 = np.float32
N_READ, FREQ, JUMP_AT = 8, 3, 4
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
def models(L, tmp_path_factory):
    """name or X -> (SvmModel, numpy model); test-written threshold models are kept for the module."""
    d = tmp_path_factory.mktemp("svm")
    made = {}

    def get(X):
        if X not in made:
            path = sr.golden(sr.MODELS["opencv3"][0]) if X == "golden" else \
                sr.write_threshold_model(str(d / f"thr_{X:.6f}.xml"), X)
            made[X] = (L.SvmModel(path), sr.read_model(path))
        return made[X]

    yield get
    for m, _ in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def stream():
    """tests/test_risk_pipeline.py's stream: a 0.6 m odometry jump that stays from reading 4 on,
    yaw-only prior poses."""
    jumps = {i: (0.0, 0.6, 0.0) for i in range(JUMP_AT, N_READ)}
    st = sy.make_stream(n_readings=N_READ, n_points=20000, seed=8, half=12.0, jumps=jumps)
    first_pose = rr.pose(0.0, st.first_origin)
    poses = [rr.pose(4.0 * (i + 1), st.origins[i]) for i in range(N_READ)]
    return st, first_pose, poses


def seq_params(L, debug, max_corr=1.0, freq=FREQ):
    return L.default_sequence_params(reference_update_frequency=freq, max_correction_magnitude=max_corr,
                                     resolution=RES, flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))


def risk_params(L):
    return L.default_risk_params(angular_view=VIEW)


def same_bits(a, b, dtype=F32):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def strip(res):
    return {k: v for k, v in res.items() if k != "rc"}


def new_session(ctx, L, model, thr, debug, max_corr=1.0, cfg=None, prefilter=True, freq=FREQ):
    from aicp_mapping_amd.session import AppSession

    return AppSession(ctx, cfg=cfg, params=seq_params(L, debug, max_corr, freq), prefilter=prefilter,
                      risk=dict(model=model, threshold=thr, params=risk_params(L)))


def feed(ctx, L, model, thr, debug, max_corr=1.0, cfg=None, between=None, session=None):
    """The stream through one risk session. Per reading: T, result, kept, record, and state(),
    reference(), reference_pose() after the call."""
    st, first_pose, poses = stream()
    s = session or new_session(ctx, L, model, thr, debug, max_corr, cfg)
    s.start(st.first, pose=first_pose)
    run = dict(T=[], out=[], kept=[], rec=[], states=[], refs=[], ref_poses=[])
    for i in range(N_READ):
        if between:
            between(i)
        T, res, kept, rec = s.process(st.readings[i], pose=poses[i])
        assert res["rc"] == 0, i
        run["T"].append(T)
        run["out"].append(strip(res))
        run["kept"].append(kept)
        run["rec"].append(rec)
        run["states"].append(s.state())
        run["refs"].append(s.reference())
        run["ref_poses"].append(s.reference_pose())
    if session is None:
        s.close()
    return run


def same_run(a, b):
    """Two session runs: every byte of what process returned and of the state after every call."""
    for i in range(N_READ):
        assert same_bits(a["T"][i], b["T"][i]), i
        assert a["out"][i] == b["out"][i] and a["kept"][i] == b["kept"][i], i
        assert bytes_of(a["rec"][i]) == bytes_of(b["rec"][i]), i
        assert same_bits(a["refs"][i][0], b["refs"][i][0]) and same_bits(a["refs"][i][1], b["refs"][i][1], np.float64), i
        assert same_bits(a["ref_poses"][i], b["ref_poses"][i], np.float64), i
        assert same_bits(a["states"][i]["initial_T"], b["states"][i]["initial_T"]), i


def bytes_of(rec):
    """A record dict's values with the floats as their bits."""
    return (rec["n_read"], rec["registered"], np.float64(rec["risk"]).tobytes()) + tuple(
        F32(rec[k]).tobytes() for k in ("fov_overlap", "octree_overlap", "alignability", "raw", "trimmed_ratio"))


def baseline(ctx, L, model, thr, debug, max_corr=1.0):
    st, first_pose, poses = stream()
    T, res, rec, done, rc = ctx.sequence_run_risk(model, thr, st.first, first_pose, st.readings, poses,
                                                  params=seq_params(L, debug, max_corr), risk_params=risk_params(L))
    assert rc == 0 and done == N_READ
    return T, res, rec


def equals_baseline(run, base):
    """Reading by reading: T bytes, every aicp_sequence_result field, every aicp_pipeline_record field."""
    T, res, rec = base
    for i in range(N_READ):
        assert same_bits(run["T"][i], T[i]), i
        assert run["out"][i] == res[i], (i, run["out"][i], res[i])
        assert same_bits(run["out"][i]["corrected_origin"], res[i]["corrected_origin"], np.float64), i
        assert bytes_of(run["rec"][i]) == bytes_of(rec[i]), (i, run["rec"][i], rec[i])
        assert run["kept"][i] == rec[i]["n_read"], i


def loop(ctx, L, ref_model, thr, debug, max_corr=1.0, cfg=None):
    st, first_pose, poses = stream()
    blocks = srr.CtxBlocks(ctx, L, ref_model, RES, risk_params(L), cfg=cfg)
    return srr.host_loop(blocks, st.first, first_pose, st.readings, poses, FREQ, max_corr, thr, debug)


def equals_loop_state(run, comp):
    """After every call: reference() bytes, reference_pose() double bytes, initialT_ bytes; and the
    decisions."""
    for i, c in enumerate(comp):
        o = run["out"][i]
        assert (o["accepted"], o["is_reference"], o["reference"], run["rec"][i]["registered"]) == \
            (c["accepted"], c["is_reference"], c["reference"], c["registered"]), i
        pts, org = run["refs"][i]
        assert same_bits(pts, c["ref"]), i
        assert same_bits(run["ref_poses"][i], c["ref_pose"], np.float64), i
        assert same_bits(org, c["ref_pose"][:3, 3], np.float64), i
        assert same_bits(run["states"][i]["initial_T"], c["initial_T"]), i
        assert run["states"][i]["reference"] == (i if c["is_reference"] else c["reference"]), i
        assert run["states"][i]["reference_points"] == len(c["ref"]) and run["states"][i]["n_processed"] == i + 1


# ---- case 1: a gate in mid-window ---------------------------------------------------------------------
_MID = {}


def mid_window(ctx, L, models, debug):
    """X from the ungated host loop, the gated host loop with its assertions, the baseline on the
    whole recording and the session's run (computed once per mode)."""
    if debug not in _MID:
        free = loop(ctx, L, models(0.0)[1], 1.0, debug)
        assert all(c["registered"] for c in free)
        ovs = [c["overlap"] for c in free]
        others = min(ovs[:JUMP_AT])
        assert others - ovs[JUMP_AT] >= 2.0, ovs
        X = 0.5 * (others + ovs[JUMP_AT])
        model, ref_model = models(X)
        comp = loop(ctx, L, ref_model, 0.5, debug)
        print("overlaps", [round(c["overlap"], 3) for c in comp], "X", X, "registered",
              [c["registered"] for c in comp], "references", [c["reference"] for c in comp])
        assert all(abs(c["overlap"] - X) >= 0.5 for c in comp)
        assert comp[JUMP_AT]["registered"] == 0
        assert comp[JUMP_AT - 1]["registered"] == 1 and comp[JUMP_AT - 1]["is_reference"] == 0
        after = [c for c in comp[JUMP_AT + 1:] if c["registered"] and c["reference"] == JUMP_AT]
        assert after and after[0]["accepted"]
        assert any(c["registered"] and c["is_reference"] for c in comp)
        _MID[debug] = dict(X=X, comp=comp, base=baseline(ctx, L, model, 0.5, debug),
                           run=feed(ctx, L, model, 0.5, debug))
    return _MID[debug]


@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
def test_gate_in_mid_window(ctx, L, models, debug):
    m = mid_window(ctx, L, models, debug)
    equals_baseline(m["run"], m["base"])
    equals_loop_state(m["run"], m["comp"])
    gated = m["run"]["out"][JUMP_AT]
    assert gated["icp"]["iterations"] == 0 and gated["status"] == 0
    assert np.array_equal(m["run"]["T"][JUMP_AT], np.eye(4, dtype=F32))
    assert same_bits(gated["corrected_origin"], m["comp"][JUMP_AT]["corrected_origin"], np.float64)


# ---- case 2: nothing gates --------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
def test_threshold_one_is_the_plain_session(ctx, L, models, debug):
    """The golden model under threshold 1.0: a plain AppSession's results on the same readings."""
    from aicp_mapping_amd.session import AppSession

    st, first_pose, poses = stream()
    run = feed(ctx, L, models("golden")[0], 1.0, debug)
    p = AppSession(ctx, params=seq_params(L, debug), prefilter=True)
    p.start(st.first, first_pose[:3, 3])
    for i in range(N_READ):
        T, res, kept = p.process(st.readings[i], poses[i][:3, 3])
        assert run["rec"][i]["registered"] == 1, i
        assert same_bits(run["T"][i], T), i
        assert run["out"][i] == strip(res), (i, run["out"][i], res)
        assert run["kept"][i] == kept, i
        assert same_bits(run["refs"][i][0], p.reference()[0]), i
        assert same_bits(run["states"][i]["initial_T"], p.state()["initial_T"]), i
    p.close()


# ---- case 3: everything gates -----------------------------------------------------------------------------
def test_threshold_zero_gates_every_reading(ctx, L, models):
    st, first_pose, poses = stream()
    run = feed(ctx, L, models("golden")[0], 0.0, False)
    assert [r["registered"] for r in run["rec"]] == [0] * N_READ and all(0.0 < r["risk"] < 1.0 for r in run["rec"])
    assert all(np.array_equal(T, np.eye(4, dtype=F32)) for T in run["T"])
    assert [(o["accepted"], o["is_reference"], o["icp"]["iterations"]) for o in run["out"]] == [(1, 1, 0)] * N_READ
    assert [o["reference"] for o in run["out"]] == [-1] + list(range(N_READ - 1))
    for i in range(N_READ):
        kept_points = ctx.prefilter(st.readings[i])
        assert same_bits(run["refs"][i][0], kept_points), i
        assert run["out"][i]["corrected_origin"] == [float(x) for x in poses[i][:3, 3]]
        assert np.array_equal(run["states"][i]["initial_T"], np.eye(4, dtype=F32))
        assert same_bits(run["ref_poses"][i], sr.fix_pitch_roll(poses[i], poses[i]), np.float64), i


# ---- case 4: the gated promotion's edges ----------------------------------------------------------------
def edge_reading(n):
    """n points of the scene cloud; the first, last and block-boundary points carry a -0.0f
    coordinate, one point a subnormal."""
    P = scene_cloud(ORIGIN_B)[:n].copy()
    for k, i in enumerate(sorted({0, n - 1} | {j for j in (255, 256, 1023, 1024, 4095, 4096) if j < n})):
        P[i, k % 3] = F32(-0.0)
    P[min(7, n - 2), 1] = np.frombuffer(np.uint32(0x00000123).tobytes(), F32)[0]
    assert np.signbit(P[0]).any() and np.signbit(P[n - 1]).any()
    return P


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4097])
def test_gated_promotion_edges(ctx, L, models, n):
    """An always-gating model (X = 1000) on pre-filtered entry: the reference after the call is the
    reading's xyz bytes, -0.0f and the subnormal included."""
    s = new_session(ctx, L, models(1000.0)[0], 0.5, False, prefilter=None)
    pa, pb = rr.pose(0.0, ORIGIN_A), rr.pose(0.0, ORIGIN_B)
    s.start(scene_cloud(ORIGIN_A)[:5000], pose=pa)
    before = s.state()
    P = edge_reading(n)
    T, res, kept, rec = s.process(P, pose=pb)
    assert rec["registered"] == 0 and res["accepted"] == 1 and res["is_reference"] == 1 and kept == n
    pts, org = s.reference()
    assert pts.tobytes() == P.tobytes()
    after = s.state()
    assert after["reference_points"] == n and after["reference"] == 0
    assert same_bits(after["initial_T"], before["initial_T"])
    assert same_bits(org, pb[:3, 3], np.float64)
    if n == 4097:  # a smaller reference behind a larger one shows no stale tail
        Q = edge_reading(255)
        T, res, kept, rec = s.process(Q, pose=pa)
        assert rec["registered"] == 0 and res["reference"] == 0 and kept == 255
        pts, _ = s.reference()
        assert pts.shape == (255, 3) and pts.tobytes() == Q.tobytes()
        assert s.state()["reference_points"] == 255 and s.state()["reference"] == 1
    s.close()


# ---- case 5: a dropped reading ------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
def test_dropped_reading(ctx, L, models, debug):
    """max_correction_magnitude 0.07 m, below the stream's drift (0.15 m along x): the readings
    registered against the first cloud are dropped, the one that jumps is gated, and those behind
    it meet it with corrections near zero and are accepted."""
    max_corr = 0.07
    X = mid_window(ctx, L, models, debug)["X"]
    model, ref_model = models(X)
    T, res, rec = base = baseline(ctx, L, model, 0.5, debug, max_corr)
    assert all(abs(q["octree_overlap"] - X) >= 0.5 for q in rec)
    dropped = [i for i in range(N_READ) if rec[i]["registered"] and not res[i]["accepted"]]
    assert dropped and any(rec[j]["registered"] and res[j]["accepted"] for j in range(dropped[0] + 1, N_READ))
    run = feed(ctx, L, model, 0.5, debug, max_corr)
    equals_baseline(run, base)
    equals_loop_state(run, loop(ctx, L, ref_model, 0.5, debug, max_corr))
    for i in dropped:
        if i == 0:
            continue
        assert same_bits(run["refs"][i][0], run["refs"][i - 1][0]), i
        assert same_bits(run["ref_poses"][i], run["ref_poses"][i - 1], np.float64), i
        assert same_bits(run["states"][i]["initial_T"], run["states"][i - 1]["initial_T"]), i
        assert run["states"][i]["reference"] == run["states"][i - 1]["reference"]
        assert run["out"][i]["corrected_origin"] == [0.0, 0.0, 0.0]
    assert any(i > 0 for i in dropped)


# ---- case 6: readings from the sweep accumulator ---------------------------------------------------------
def test_readings_from_the_accumulator(ctx, L, models):
    """process(acc, pose=) reads the accumulator's cloud where it lies: the bits of a twin session fed
    getCloud()'s rows; the accumulator is unchanged, then cleared and refilled straight after."""
    from aicp_mapping_amd.accumulator import SweepAccumulator
    from test_session import fill, scene_sweeps

    cap = max(sum(len(s) for s in scene_sweeps(k)[0]) for k in range(4))
    acc = SweepAccumulator(ctx, cap, batch_size=3)
    model = models(0.0)[0]  # (raw = overlap >= 0: risk <= 0.5, the gate stays open)
    a = new_session(ctx, L, model, 0.5, True, freq=2)
    b = new_session(ctx, L, model, 0.5, True, freq=2)
    o0 = fill(acc, 0)
    first = acc.getCloud()
    a.start(acc, pose=rr.pose(0.0, o0))
    b.start(first, pose=rr.pose(0.0, o0))
    assert same_bits(a.reference()[0], b.reference()[0]) and same_bits(acc.getCloud(), first)
    registered = []
    for k in (1, 2, 3):
        acc.clear()
        o = fill(acc, k)
        cloud = acc.getCloud()
        P = rr.pose(1.0 * k, o)
        Ta, ra, ka, qa = a.process(acc, pose=P)
        assert same_bits(acc.getCloud(), cloud)  # left as it is
        acc.clear()
        fill(acc, (k + 1) % 4)  # the node's next reading starts at once
        Tb, rb, kb, qb = b.process(cloud, pose=P)
        assert same_bits(Ta, Tb) and ra == rb and ka == kb and bytes_of(qa) == bytes_of(qb), k
        assert ra["status"] == 0 and 50 <= ka < len(cloud)
        assert same_bits(a.reference()[0], b.reference()[0]), k
        assert same_bits(a.reference_pose(), b.reference_pose(), np.float64), k
        assert same_bits(a.state()["initial_T"], b.state()["initial_T"]), k
        registered.append(qa["registered"])
    assert any(registered)
    for s in (a, b):
        s.close()
    acc.free()


# ---- case 7: interleaving -------------------------------------------------------------------------------------
def test_other_calls_between_readings_change_nothing(ctx, L, models):
    m = mid_window(ctx, L, models, False)
    model, _ = models(m["X"])
    A, B = scene_cloud(ORIGIN_A)[:20000], scene_cloud(ORIGIN_B)[:20000]
    pa, pb = rr.pose(0.0, ORIGIN_A), rr.pose(0.0, ORIGIN_B)
    other = sy.make_pair(3000, 3000, seed=5)
    st = stream()[0]

    def between(i):
        ctx.alignment_features(A, B, pa, pb, risk_params(L))
        ctx.prefilter(st.readings[(i + 3) % N_READ])
        ctx.svm_predict(models("golden")[0], [[50.0, 0.5], [10.0, 0.1]])
        ctx.register(other.ref, other.read)

    same_run(feed(ctx, L, model, 0.5, False, between=between), m["run"])


def test_risk_and_plain_sessions_alternate(ctx, L, models):
    from aicp_mapping_amd.session import AppSession

    st, first_pose, poses = stream()
    m = mid_window(ctx, L, models, True)
    model, _ = models(m["X"])
    solo = AppSession(ctx, params=seq_params(L, False), prefilter=True)
    solo.start(st.first, st.first_origin)
    plain_solo = [solo.process(st.readings[i], st.origins[i]) for i in range(N_READ)]
    solo.close()
    p = AppSession(ctx, params=seq_params(L, False), prefilter=True)
    p.start(st.first, st.first_origin)
    got = []

    def between(i):
        got.append(p.process(st.readings[i], st.origins[i]))

    same_run(feed(ctx, L, model, 0.5, True, between=between), m["run"])
    p.close()
    for (Ta, ra, ka), (Tb, rb, kb) in zip(got, plain_solo):
        assert same_bits(Ta, Tb) and ra == rb and ka == kb


@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
def test_two_runs_are_identical(ctx, L, models, debug):
    m = mid_window(ctx, L, models, debug)
    same_run(feed(ctx, L, models(m["X"])[0], 0.5, debug), m["run"])


# ---- case 8: a point-to-point chain ---------------------------------------------------------------------------
def test_point_to_point_chain(ctx, L, models):
    """knn_normals = 0 runs in the risk session (aicp_hip_sequence_run_risk refuses it): the host
    loop with that chain, T, decisions and references exact."""
    cfg = L.default_config(point_to_point=True)
    X = mid_window(ctx, L, models, False)["X"]
    model, ref_model = models(X)
    comp = loop(ctx, L, ref_model, 0.5, False, cfg=cfg)
    assert all(abs(c["overlap"] - X) >= 0.5 for c in comp)
    assert any(c["registered"] == 0 for c in comp) and any(c["registered"] and c["iterations"] > 0 for c in comp)
    run = feed(ctx, L, model, 0.5, False, cfg=cfg)
    equals_loop_state(run, comp)
    for i, c in enumerate(comp):
        assert same_bits(run["T"][i], c["T"]), i
        assert run["out"][i]["icp"]["iterations"] == c["iterations"] and run["kept"][i] == c["kept"], i
        assert F32(run["rec"][i]["octree_overlap"]) == F32(c["overlap"]), i
        assert F32(run["rec"][i]["alignability"]) == F32(c["alignability"]), i
        if c["accepted"]:
            assert same_bits(run["out"][i]["corrected_origin"], c["corrected_origin"], np.float64), i
    st, first_pose, poses = stream()
    *_, rc = ctx.sequence_run_risk(model, 0.5, st.first, first_pose, st.readings, poses, cfg=cfg,
                                   params=seq_params(L, False), risk_params=risk_params(L), raise_on_error=False)
    assert rc == L.AICP_ERR_UNSUPPORTED


# ---- case 9: endings and arguments ------------------------------------------------------------------------------
def test_emptied_reading_ends_the_session_and_start_pose_revives_it(ctx, L, models):
    st, first_pose, poses = stream()
    s = new_session(ctx, L, models("golden")[0], 1.0, True)
    s.start(st.first, pose=first_pose)
    first2 = [s.process(st.readings[i], pose=poses[i]) for i in range(2)]
    before, ref_before, pose_before = s.state(), s.reference()[0], s.reference_pose()
    T, res, kept, rec = s.process(rs.scattered(), pose=poses[2], raise_on_error=False)
    assert res["rc"] == L.AICP_ERR_INVALID and res["status"] == L.AICP_ERR_INVALID and kept == 0
    assert not res["accepted"] and np.array_equal(T, np.eye(4, dtype=F32)) and rec["registered"] == 0
    after = s.state()
    assert after["ended"] and after["n_processed"] == 3 and after["reference"] == before["reference"]
    assert same_bits(after["initial_T"], before["initial_T"]) and same_bits(s.reference()[0], ref_before)
    assert same_bits(s.reference_pose(), pose_before, np.float64)
    with pytest.raises(L.AicpError) as e:
        s.process(st.readings[3], pose=poses[3])
    assert e.value.code == L.AICP_ERR_INVALID and "ended at reading 2" in str(e.value)
    s.start(st.first, pose=first_pose)
    state = s.state()
    assert not state["ended"] and state["n_processed"] == 0 and state["reference"] == -1
    again = s.process(st.readings[0], pose=poses[0])
    assert same_bits(again[0], first2[0][0]) and again[1] == first2[0][1] and again[2] == first2[0][2]
    assert bytes_of(again[3]) == bytes_of(first2[0][3])
    s.close()


def test_registration_error_ends_the_session(ctx, L, models):
    """tests/test_session.py's case: reading 6, 200 m away with a 5 m matcher radius, under a gate
    that never closes."""
    st = sy.make_stream(n_readings=8, n_points=4000, seed=9, half=15.0)
    st.readings[6] = (st.readings[6] + F32(200.0)).astype(F32)
    st.origins[6] = st.origins[6] + 200.0
    cfg = L.default_config(nn_max_dist=5.0)
    s = new_session(ctx, L, models(0.0)[0], 1.0, False, cfg=cfg, prefilter=None, freq=5)
    s.start(st.first, pose=rr.pose(0.0, st.first_origin))
    for i in range(6):
        T, res, kept, rec = s.process(st.readings[i], pose=rr.pose(0.0, st.origins[i]))
        assert res["status"] == 0 and rec["registered"] == 1
    before, ref_before, pose_before = s.state(), s.reference()[0], s.reference_pose()
    T, res, kept, rec = s.process(st.readings[6], pose=rr.pose(0.0, st.origins[6]), raise_on_error=False)
    assert res["rc"] == L.AICP_ERR_CONVERGENCE and res["status"] == L.AICP_ERR_CONVERGENCE and not res["accepted"]
    assert rec["registered"] == 1 and res["reference"] == before["reference"]
    after = s.state()
    assert after["ended"] and after["n_processed"] == 7 and after["reference"] == before["reference"]
    assert same_bits(after["initial_T"], before["initial_T"]) and same_bits(s.reference()[0], ref_before)
    assert same_bits(s.reference_pose(), pose_before, np.float64)
    with pytest.raises(L.AicpError) as e:
        s.process(st.readings[7], pose=rr.pose(0.0, st.origins[7]))
    assert e.value.code == L.AICP_ERR_INVALID
    s.close()


def test_invalid_arguments_and_handle_kinds(ctx, L, models):
    from aicp_mapping_amd.session import AppSession

    lib = L.lib
    model = models(1000.0)[0]
    rp, cfg = risk_params(L), L.default_config()
    h = C.c_void_p()
    for bad in (dict(reference_update_frequency=0), dict(resolution=0.0), dict(resolution=-1.0), dict(flags=64)):
        prm = L.default_sequence_params(**bad)
        assert lib.aicp_hip_session_create_risk(ctx.h, C.byref(cfg), C.byref(prm), None, C.byref(rp), model.h, 0.5,
                                                C.byref(h)) == L.AICP_ERR_INVALID and not h.value
    prm = seq_params(L, False)
    assert lib.aicp_hip_session_create_risk(ctx.h, C.byref(cfg), C.byref(prm), None, None, model.h, 0.5,
                                            C.byref(h)) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_session_create_risk(ctx.h, C.byref(cfg), C.byref(prm), None, C.byref(rp), None, 0.5,
                                            C.byref(h)) == L.AICP_ERR_INVALID
    A = scene_cloud(ORIGIN_A)[:3000]
    B = scene_cloud(ORIGIN_B)[:3000]
    pa, pb = rr.pose(0.0, ORIGIN_A), rr.pose(0.0, ORIGIN_B)
    r = new_session(ctx, L, model, 0.5, False, prefilter=None)
    p = AppSession(ctx, params=seq_params(L, False))
    r.start(A, pose=pa)
    p.start(A, pa[:3, 3])
    T, res, rec = np.zeros(16, F32), L.SequenceResult(), L.PipelineRecord()
    c, keep = L.make_cloud(B, pb[:3, 3])
    pose = L._pose16(pb)
    INV = L.AICP_ERR_INVALID

    def untouched(s, state, ref):
        now = s.state()
        return {k: v for k, v in now.items() if k != "initial_T"} == {k: v for k, v in state.items() if k != "initial_T"} \
            and same_bits(now["initial_T"], state["initial_T"]) and same_bits(s.reference()[0], ref)

    rs0, rref, ps0, pref = r.state(), r.reference()[0], p.state(), p.reference()[0]
    rpose0 = r.reference_pose()
    # the wrong call for the handle's kind
    assert lib.aicp_hip_session_process(ctx.h, r.h, C.byref(c), L._fptr(T), C.byref(res), None) == INV
    assert lib.aicp_hip_session_process_accum(ctx.h, r.h, r.h, L._dptr(pose), L._fptr(T), C.byref(res), None) == INV
    assert lib.aicp_hip_session_start(ctx.h, r.h, C.byref(c)) == INV
    assert lib.aicp_hip_session_start_accum(ctx.h, r.h, r.h, L._dptr(pose)) == INV
    assert lib.aicp_hip_session_process_risk(ctx.h, p.h, C.byref(c), L._dptr(pose), L._fptr(T), C.byref(res),
                                             C.byref(rec), None) == INV
    assert lib.aicp_hip_session_process_accum_risk(ctx.h, p.h, p.h, L._dptr(pose), L._fptr(T), C.byref(res),
                                                   C.byref(rec), None) == INV
    assert lib.aicp_hip_session_start_pose(ctx.h, p.h, C.byref(c), L._dptr(pose)) == INV
    assert lib.aicp_hip_session_start_accum_pose(ctx.h, p.h, p.h, L._dptr(pose)) == INV
    assert lib.aicp_hip_session_reference_pose(ctx.h, p.h, L._dptr(pose.copy())) == INV
    # NULL arguments
    assert lib.aicp_hip_session_process_risk(ctx.h, r.h, C.byref(c), None, L._fptr(T), C.byref(res), C.byref(rec),
                                             None) == INV
    assert lib.aicp_hip_session_process_risk(ctx.h, r.h, C.byref(c), L._dptr(pose), L._fptr(T), C.byref(res), None,
                                             None) == INV
    assert lib.aicp_hip_session_process_risk(ctx.h, r.h, None, L._dptr(pose), L._fptr(T), C.byref(res), C.byref(rec),
                                             None) == INV
    assert lib.aicp_hip_session_process_risk(ctx.h, r.h, C.byref(c), L._dptr(pose), None, C.byref(res), C.byref(rec),
                                             None) == INV
    assert lib.aicp_hip_session_process_accum_risk(ctx.h, r.h, None, L._dptr(pose), L._fptr(T), C.byref(res),
                                                   C.byref(rec), None) == INV
    assert lib.aicp_hip_session_start_pose(ctx.h, r.h, C.byref(c), None) == INV
    assert lib.aicp_hip_session_start_accum_pose(ctx.h, r.h, None, L._dptr(pose)) == INV
    assert lib.aicp_hip_session_reference_pose(ctx.h, r.h, None) == INV
    assert untouched(r, rs0, rref) and untouched(p, ps0, pref)
    assert same_bits(r.reference_pose(), rpose0, np.float64)
    with pytest.raises(TypeError):
        r.process(B, pb[:3, 3])
    with pytest.raises(TypeError):
        p.process(B, pose=pb)
    # both still work
    assert lib.aicp_hip_session_process_risk(ctx.h, r.h, C.byref(c), L._dptr(pose), L._fptr(T), C.byref(res),
                                             C.byref(rec), None) == L.AICP_OK
    assert rec.registered == 0 and r.state()["n_processed"] == 1 and r.state()["reference"] == 0
    assert p.process(B, pb[:3, 3])[1]["status"] == 0
    # before start
    q = new_session(ctx, L, model, 0.5, False, prefilter=None)
    for call in (lambda: q.process(B, pose=pb), q.reference_pose, q.state):
        with pytest.raises(L.AicpError) as e:
            call()
        assert e.value.code == INV
    for s in (r, p, q):
        s.close()
