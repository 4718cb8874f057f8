"""failure_prediction_mode on the device: one pair through the gated pipeline (aicp_hip_pipeline)
and App's frame-to-reference stream with the gate (aicp_hip_sequence_run_risk), against hand
compositions of the existing calls (overlap, alignment_features, align_batch, prefilter, transform),
the numpy classifier of tests/svm_reference.py and its policy state machine.

A test-written degree-1 model (gamma 1, coef0 0, one support vector (1, 0), alpha 1, rho X) has
raw = overlap - X, so risk > 0.5 <=> overlap < X: X places the gate. Every gap between X and an
overlap the decision depends on is asserted on the composition before the device's stream or
pipeline is looked at. raw and risk are held to the bars of tests/test_svm.py."""
import numpy as np
import pytest

import svm_reference as sr
from aicp_mapping_amd import synthetic as sy
from test_alignment_risk import ORIGIN_A, ORIGIN_B, scene_cloud, settle_pose  # the scene pair, its poses
import risk_reference as rr

pytestmark = pytest.mark.gpu

RES = float(np.float32(0.2))
VIEW = 270.0


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def threshold_model(L, tmp_path, X):
    path = sr.write_threshold_model(str(tmp_path / f"thr_{X:.4f}.xml"), X)
    return L.SvmModel(path), sr.read_model(path)


def check_classifier(rec, ref_model, ov, al):
    raw, risk, terms = sr.predict(ref_model, np.array([[ov, al]], np.float32))
    bar = sr.raw_bar(raw, terms)[0]
    assert abs(float(rec["raw"]) - float(raw[0])) <= bar, (rec["raw"], raw[0], bar)
    assert abs(rec["risk"] - risk[0]) <= 0.25 * bar + 1e-15, (rec["risk"], risk[0])
    return risk[0]


# ---- one pair ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(ctx, L):
    """The scene pair, its poses settled, and the hand composition's parts (computed once)."""
    A, B = scene_cloud(ORIGIN_A), scene_cloud(ORIGIN_B)
    pa, pb = rr.pose(0.0, ORIGIN_A), rr.pose(0.0, ORIGIN_B)
    pb, pa = settle_pose(A, pb, 100.0, VIEW), settle_pose(B, pa, 100.0, VIEW)
    prm = L.default_risk_params(angular_view=VIEW)
    ov = ctx.overlap(A, B, pa[:3, 3], pb[:3, 3], RES)
    feats = ctx.alignment_features(A, B, pa, pb, prm)
    T, st, rc = ctx.align_batch([dict(ref=A, read=B, ref_origin=pa[:3, 3], read_origin=pb[:3, 3])],
                                flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP, resolution=RES)
    assert rc == 0 and st[0]["iterations"] > 0 and np.float32(st[0]["overlap_percent"]) == np.float32(ov)
    return dict(A=A, B=B, pa=pa, pb=pb, prm=prm, ov=ov, feats=feats, T=T[0], st=st[0])


X_BELOW, X_ABOVE = 10.0, 99.0


def test_pipeline_registers_below_the_gate(ctx, L, pair, tmp_path):
    p = pair
    assert p["ov"] - X_BELOW > 5.0                       # well above X: risk < 0.5
    model, ref_model = threshold_model(L, tmp_path, X_BELOW)
    T, rec, st = ctx.pipeline(model, 0.5, p["A"], p["B"], p["pa"], p["pb"], risk_params=p["prm"], resolution=RES)
    assert rec["registered"] == 1 and rec["n_read"] == len(p["B"])
    assert np.float32(rec["octree_overlap"]).tobytes() == np.float32(p["ov"]).tobytes()
    assert np.float32(rec["alignability"]).tobytes() == np.float32(p["feats"]["alignability"]).tobytes()
    assert np.float32(rec["fov_overlap"]).tobytes() == np.float32(p["feats"]["fov_overlap"]).tobytes()
    assert T.tobytes() == p["T"].tobytes()
    for k in ("status", "iterations", "converged", "trimmed_ratio", "overlap_percent", "overlap_keys",
              "nn_points_touched", "nn_nodes_touched"):
        assert st[k] == p["st"][k], k
    assert np.float32(rec["trimmed_ratio"]) == np.float32(L.autotune_ratio(p["ov"])) == np.float32(st["trimmed_ratio"])
    risk = check_classifier(rec, ref_model, p["ov"], p["feats"]["alignability"])
    assert risk < 0.5
    # the features and the overlap calls themselves are not disturbed
    assert ctx.overlap(p["A"], p["B"], p["pa"][:3, 3], p["pb"][:3, 3], RES) == p["ov"]
    assert ctx.alignment_features(p["A"], p["B"], p["pa"], p["pb"], p["prm"])["alignability"] == \
        p["feats"]["alignability"]
    model.close()


def test_pipeline_gates_above(ctx, L, pair, tmp_path):
    p = pair
    assert X_ABOVE - p["ov"] > 5.0                       # well below X: risk > 0.5
    model, ref_model = threshold_model(L, tmp_path, X_ABOVE)
    T, rec, st = ctx.pipeline(model, 0.5, p["A"], p["B"], p["pa"], p["pb"], risk_params=p["prm"], resolution=RES)
    assert rec["registered"] == 0
    assert np.array_equal(T, np.eye(4, dtype=np.float32))
    assert st["iterations"] == 0 and st["status"] == 0
    assert np.float32(rec["octree_overlap"]).tobytes() == np.float32(p["ov"]).tobytes()
    assert np.float32(rec["alignability"]).tobytes() == np.float32(p["feats"]["alignability"]).tobytes()
    assert st["overlap_keys"] == p["st"]["overlap_keys"]
    assert check_classifier(rec, ref_model, p["ov"], p["feats"]["alignability"]) > 0.5
    # the same model under threshold 1.0 registers: the gate is the comparison, nothing else
    T1, rec1, _ = ctx.pipeline(model, 1.0, p["A"], p["B"], p["pa"], p["pb"], risk_params=p["prm"], resolution=RES)
    assert rec1["registered"] == 1 and T1.tobytes() == p["T"].tobytes() and rec1["risk"] == rec["risk"]
    model.close()


def test_pipeline_with_the_golden_model(ctx, L, pair):
    p = pair
    path = sr.golden(sr.MODELS["opencv3"][0])
    model, ref_model = L.SvmModel(path), sr.read_model(path)
    T, rec, st = ctx.pipeline(model, 0.5, p["A"], p["B"], p["pa"], p["pb"], risk_params=p["prm"], resolution=RES)
    risk = check_classifier(rec, ref_model, p["ov"], p["feats"]["alignability"])
    assert abs(risk - 0.5) > 1e-4                         # (the decision does not hang on the last bits)
    assert rec["registered"] == int(risk <= 0.5)
    assert (T.tobytes() == p["T"].tobytes()) if rec["registered"] else np.array_equal(T, np.eye(4))
    model.close()


# ---- the stream -------------------------------------------------------------------------------
N_READ, FREQ, JUMP_AT = 8, 3, 4


@pytest.fixture(scope="module")
def stream():
    """make_stream as test_sequence_raw_* use it, with an odometry jump that stays from reading
    JUMP_AT on (mid-window: readings 0-2 end the first window, 3 is the second window's first), and
    yaw-only prior poses."""
    jumps = {i: (0.0, 0.6, 0.0) for i in range(JUMP_AT, N_READ)}
    st = sy.make_stream(n_readings=N_READ, n_points=20000, seed=8, half=12.0, jumps=jumps)
    first_pose = rr.pose(0.0, st.first_origin)
    poses = [rr.pose(4.0 * (i + 1), st.origins[i]) for i in range(N_READ)]
    return st, first_pose, poses


def apply4(T, P):
    """pcl::transformPointCloud as the library's host code does it: float, term by term."""
    T = np.asarray(T, np.float32)
    P = np.asarray(P, np.float32)
    out = np.empty_like(P)
    for r in range(3):
        s = T[r, 0] * P[:, 0]
        s = s + T[r, 1] * P[:, 1]
        s = s + T[r, 2] * P[:, 2]
        out[:, r] = s + T[r, 3]
    return out


def compose(ctx, L, stream, ref_model, thr, debug, rp):
    """The stream, reading by reading, from the existing calls, the numpy classifier and the policy."""
    st, first_pose, poses = stream
    ref = ctx.prefilter(st.first)
    ref_pose = sr.fix_pitch_roll(first_pose, first_pose)
    policy = sr.GatePolicy(FREQ, 1.0, thr)
    out = []
    for i in range(N_READ):
        odom = poses[i]
        prior = sr.moved_pose(policy.initT, odom) if debug else odom.copy()
        raw_cloud = ctx.transform(policy.initT, st.readings[i]) if debug else st.readings[i]
        rd = ctx.prefilter(raw_cloud)
        ov = ctx.overlap(ref, rd, ref_pose[:3, 3], prior[:3, 3], RES)
        feats = ctx.alignment_features(ref, rd, ref_pose, prior, rp)
        _, risk, _ = sr.predict(ref_model, np.array([[ov, feats["alignability"]]], np.float32))
        T, iters = np.eye(4, dtype=np.float32), 0
        if not policy.gated(risk[0]):
            Ts, sts, rc = ctx.align_batch([dict(ref=ref, read=rd, ref_origin=ref_pose[:3, 3], read_origin=prior[:3, 3])],
                                          flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP, resolution=RES)
            assert rc == 0
            T, iters = Ts[0], sts[0]["iterations"]
        d = policy.step(i, risk[0], T)
        d.update(T=T, overlap=ov, alignability=feats["alignability"], risk=risk[0], kept=len(rd), iterations=iters,
                 corrected_origin=None)
        if not d["registered"]:
            d["corrected_origin"] = prior[:3, 3].copy()
            ref, ref_pose = rd, sr.fix_pitch_roll(prior, odom)
        elif d["accepted"]:
            corrected = sr.moved_pose(T, prior)
            d["corrected_origin"] = corrected[:3, 3].copy()
            if d["is_reference"]:
                ref, ref_pose = apply4(T, rd), sr.fix_pitch_roll(corrected, odom)
        out.append(d)
    return out


def run_stream(ctx, L, stream, model, thr, debug, rp):
    st, first_pose, poses = stream
    prm = L.default_sequence_params(reference_update_frequency=FREQ, max_correction_magnitude=1.0, resolution=RES,
                                    flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))
    return ctx.sequence_run_risk(model, thr, st.first, first_pose, st.readings, poses, params=prm, risk_params=rp)


def check_stream(got, comp):
    T, res, rec, done, rc = got
    assert rc == 0 and done == N_READ
    for i, (r, q, c) in enumerate(zip(res, rec, comp)):
        assert T[i].tobytes() == c["T"].tobytes(), i
        assert (r["status"], r["accepted"], r["is_reference"], r["reference"]) == \
            (0, c["accepted"], c["is_reference"], c["reference"]), i
        assert q["registered"] == c["registered"] and q["n_read"] == c["kept"], i
        assert np.float32(q["octree_overlap"]) == np.float32(c["overlap"]), i
        assert np.float32(q["alignability"]) == np.float32(c["alignability"]), i
        assert r["icp"]["iterations"] == c["iterations"], i
        if c["accepted"]:
            assert np.array_equal(np.array(r["corrected_origin"]), c["corrected_origin"]), i
        else:
            assert r["corrected_origin"] == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_stream_with_a_gate_in_mid_window(ctx, L, stream, tmp_path, debug):
    rp = L.default_risk_params(angular_view=VIEW)
    # X from the ungated composition: between the overlap of the reading that jumps and the
    # overlaps before it (ungated, the readings behind it meet references in the old frame and stay
    # low; gated, they meet the jumped reading itself: the gap is asserted on that composition below)
    free_model = sr.read_model(sr.write_threshold_model(str(tmp_path / "free.xml"), 0.0))
    free = compose(ctx, L, stream, free_model, 1.0, debug, rp)
    assert all(c["registered"] for c in free)
    ovs = [c["overlap"] for c in free]
    others = min(ovs[:JUMP_AT])
    assert others - ovs[JUMP_AT] >= 2.0, ovs
    X = 0.5 * (others + ovs[JUMP_AT])
    model, ref_model = threshold_model(L, tmp_path, X)
    comp = compose(ctx, L, stream, ref_model, 0.5, debug, rp)
    print("overlaps", [round(c["overlap"], 3) for c in comp], "X", X, "registered", [c["registered"] for c in comp],
          "references", [c["reference"] for c in comp])
    assert all(abs(c["overlap"] - X) >= 0.5 for c in comp)           # the gap, on both sides
    assert comp[JUMP_AT]["registered"] == 0 and comp[JUMP_AT - 1]["registered"] == 1 and \
        comp[JUMP_AT - 1]["is_reference"] == 0                        # gated in mid-window
    after = [c for c in comp[JUMP_AT + 1:] if c["registered"] and c["reference"] == JUMP_AT]
    assert after and after[0]["accepted"]                             # registered against the gated reference
    assert any(c["registered"] and c["is_reference"] for c in comp)   # a frequency update
    check_stream(run_stream(ctx, L, stream, model, 0.5, debug, rp), comp)
    model.close()


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_stream_threshold_one_is_the_raw_stream(ctx, L, stream, debug):
    """Nothing gates under threshold 1.0: aicp_hip_sequence_run_raw's results bit for bit."""
    st, first_pose, poses = stream
    rp = L.default_risk_params(angular_view=VIEW)
    model = L.SvmModel(sr.golden(sr.MODELS["opencv3"][0]))
    T, res, rec, done, rc = run_stream(ctx, L, stream, model, 1.0, debug, rp)
    prm = L.default_sequence_params(reference_update_frequency=FREQ, max_correction_magnitude=1.0, resolution=RES,
                                    flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))
    T0, res0, done0, rc0 = ctx.sequence_run(st.first, st.first_origin, st.readings, st.origins, params=prm,
                                            prefilter=True)
    assert (rc, done) == (rc0, done0) == (0, N_READ)
    assert T.tobytes() == T0.tobytes()
    assert all(q["registered"] == 1 for q in rec)
    for a, b in zip(res, res0):
        for k in ("status", "accepted", "reference", "is_reference", "corrected_origin"):
            assert a[k] == b[k], k
        for k in ("iterations", "trimmed_ratio", "overlap_percent", "overlap_keys"):
            assert a["icp"][k] == b["icp"][k], k
    model.close()


def test_stream_threshold_zero_registers_nothing(ctx, L, stream):
    """Every risk of the golden model is above 0: every reading is gated and becomes the reference."""
    st, first_pose, poses = stream
    rp = L.default_risk_params(angular_view=VIEW)
    model = L.SvmModel(sr.golden(sr.MODELS["opencv3"][0]))
    T, res, rec, done, rc = run_stream(ctx, L, stream, model, 0.0, False, rp)
    assert rc == 0 and done == N_READ
    assert all(np.array_equal(t, np.eye(4, dtype=np.float32)) for t in T)
    assert [q["registered"] for q in rec] == [0] * N_READ and all(0.0 < q["risk"] < 1.0 for q in rec)
    assert [(r["accepted"], r["is_reference"], r["icp"]["iterations"]) for r in res] == [(1, 1, 0)] * N_READ
    assert [r["reference"] for r in res] == [-1] + list(range(N_READ - 1))
    for r, P in zip(res, poses):
        assert r["corrected_origin"] == [float(x) for x in P[:3, 3]]
    model.close()
