"""The failure-prediction classifier without a device: the restatement (tests/svm_reference.py)
against the reference's own recordings, the library's model reader (aicp_hip_svm_load / _info)
against the restatement's, its refusals, and the gated stream policy as a state machine. The GPU side
is tests/test_svm.py and tests/test_risk_pipeline.py.

Recordings (tests/golden/svm): probs_opencv3.txt and probs_27Aug.txt are what the reference's
classifier printed, with 6 significant digits, for the 269 inputs of testing_labelled_27Aug.txt
under the two golden models. Bar for the restatement: svm_reference.recorded_bar, the print rounding
plus the float roundings of raw and of every K through the logistic (slope <= 1/4), computed from the
restatement's own alpha and K."""
import ctypes as C

import numpy as np
import pytest

import svm_reference as sr


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def inputs():
    X = sr.read_inputs()
    assert X.shape == (269, 2)
    return X


@pytest.mark.parametrize("name", sorted(sr.MODELS))
def test_restatement_reproduces_the_recording(inputs, name):
    model_file, probs_file, n_above = sr.MODELS[name]
    m = sr.read_model(sr.golden(model_file))
    rec, texts = sr.read_probs(sr.golden(probs_file))
    assert len(rec) == 269
    raw, risk, terms = sr.predict(m, inputs)
    err = np.abs(risk - rec)
    bar = sr.recorded_bar(raw, terms, texts)
    print(f"{name}: restatement vs recording max {err.max():.3g}, bar max {bar.max():.3g}, "
          f"closest recorded value to 0.5: {np.abs(rec - 0.5).min():.3g}")
    assert (err <= bar).all(), (err.max(), bar[np.argmax(err - bar)])
    assert np.array_equal(risk > 0.5, rec > 0.5)
    assert int((rec > 0.5).sum()) == n_above
    assert np.array_equal(sr.gate(risk, 0.5), rec > 0.5)


@pytest.mark.parametrize("name", sorted(sr.MODELS))
def test_library_reads_the_golden_models(L, name):
    path = sr.golden(sr.MODELS[name][0])
    ref = sr.read_model(path)
    assert (ref["svm_type"], ref["kernel"]) == ("C_SVC", "POLY")
    m = L.SvmModel(path)
    got = m.info()
    m.close()
    for k in ("format", "var_count", "class_count", "sv_total", "sv_count", "has_index", "degree", "gamma", "coef0",
              "rho"):
        assert got[k] == ref[k], k
    assert np.array_equal(got["support_vectors"].view(np.uint32), ref["support_vectors"].view(np.uint32))
    assert np.array_equal(got["alpha"], ref["alpha"])
    assert np.array_equal(got["index"], ref["index"])
    assert ref["format"] == (3 if name == "opencv3" else 0)
    if name == "opencv3":  # its decision function visits the support vectors out of order
        assert ref["sv_count"] == 200 and not np.array_equal(ref["index"], np.arange(200))


def test_library_reads_a_model_without_index(L, tmp_path):
    sv = np.array([[1.5, 2.0], [3.0, 0.25], [0.5, 7.0]], np.float32)
    for fmt in (3, 0):
        p = sr.write_model(str(tmp_path / f"m{fmt}.xml"), sv, [0.5, -0.25, 0.125], 0.1, 2.5, 0.01, 0.3, index=None,
                           fmt=fmt)
        ref = sr.read_model(p)
        got = L.SvmModel(p).info()
        assert got["has_index"] == 0 and got["format"] == fmt
        assert np.array_equal(got["index"], [0, 1, 2]) and np.array_equal(ref["index"], [0, 1, 2])
        assert np.array_equal(got["support_vectors"], sv) and np.array_equal(got["alpha"], ref["alpha"])
        assert (got["degree"], got["gamma"], got["coef0"], got["rho"]) == (2.5, 0.01, 0.3, 0.1)


def _load_rc(L, path):
    h = C.c_void_p()
    rc = L.lib.aicp_hip_svm_load(str(path).encode(), C.byref(h))
    assert (rc == 0) == bool(h.value)
    if h.value:
        L.lib.aicp_hip_svm_free(h)
    return rc


def test_library_refuses_what_it_does_not_serve(L, tmp_path):
    sv2 = [[1.0, 2.0], [3.0, 4.0]]
    ok = sr.write_model(str(tmp_path / "ok.xml"), sv2, [1.0, -1.0], 0.5, 3.0, 1.0, 0.0)
    assert _load_rc(L, ok) == L.AICP_OK
    cases = {
        "rbf": (dict(kernel="RBF"), L.AICP_ERR_UNSUPPORTED),
        "nu_svc": (dict(svm_type="NU_SVC"), L.AICP_ERR_UNSUPPORTED),
        "three_classes": (dict(class_count=3), L.AICP_ERR_UNSUPPORTED),
        "index_out_of_range": (dict(index=[0, 2]), L.AICP_ERR_INVALID),
        "index_negative": (dict(index=[0, -1]), L.AICP_ERR_INVALID),
        "sv_count_not_alpha": (dict(sv_count=3), L.AICP_ERR_INVALID),
        "sv_total_not_rows": (dict(sv_total=3), L.AICP_ERR_INVALID),
        "truncated": (dict(truncate=len(open(ok).read()) // 2), L.AICP_ERR_INVALID),
    }
    for name, (kw, want) in cases.items():
        p = sr.write_model(str(tmp_path / f"{name}.xml"), sv2, [1.0, -1.0], 0.5, 3.0, 1.0, 0.0, **kw)
        assert _load_rc(L, p) == want, name
    p = sr.write_model(str(tmp_path / "var3.xml"), [[1.0, 2.0, 3.0]], [1.0], 0.5, 3.0, 1.0, 0.0)
    assert _load_rc(L, p) == L.AICP_ERR_UNSUPPORTED
    assert _load_rc(L, tmp_path / "missing.xml") == L.AICP_ERR_INVALID
    (tmp_path / "text.xml").write_text("not a model\n")
    assert _load_rc(L, tmp_path / "text.xml") == L.AICP_ERR_INVALID
    with pytest.raises(L.AicpError) as e:
        L.SvmModel(str(tmp_path / "rbf.xml"))
    assert e.value.code == L.AICP_ERR_UNSUPPORTED


def test_struct_layouts(L):
    assert C.sizeof(L.SvmInfo) == 56 and C.sizeof(L.PipelineRecord) == 40
    assert L.PipelineRecord.risk.offset == 24 and L.PipelineRecord.registered.offset == 32


# ---- the stream policy (app.cpp:362-414) ---------------------------------------------------------
def _T(tx=0.0, ty=0.0):
    T = np.eye(4, dtype=np.float32)
    T[0, 3], T[1, 3] = tx, ty
    return T


def run_policy(script, F=3, max_corr=0.5, thr=0.5):
    p = sr.GatePolicy(F, max_corr, thr)
    return [p.step(i, risk, T) for i, (risk, T) in enumerate(script)], p


def test_policy_gate_in_mid_window_restarts_the_count():
    # F = 3: without the gate readings 2 and 5 become references; a gate at reading 1 makes it the
    # reference at once and the next frequency update falls on reading 4
    plain, _ = run_policy([(0.1, _T(0.01))] * 6)
    assert [i for i, r in enumerate(plain) if r["is_reference"]] == [2, 5]
    assert [r["reference"] for r in plain] == [-1, -1, -1, 2, 2, 2]
    script = [(0.1, _T(0.01)), (0.9, None)] + [(0.1, _T(0.01))] * 5
    out, p = run_policy(script)
    assert [r["registered"] for r in out] == [1, 0, 1, 1, 1, 1, 1]
    assert [r["accepted"] for r in out] == [1] * 7
    assert [i for i, r in enumerate(out) if r["is_reference"]] == [1, 4]
    assert [r["reference"] for r in out] == [-1, -1, 1, 1, 1, 4, 4]
    assert p.graph == [-1, 0, 1, 2, 3, 4, 5, 6]
    # the gated reading leaves initialT_ alone: six corrections of 0.01 m went in
    assert abs(p.initT[0, 3] - 0.06) < 1e-6


def test_policy_drop_adds_nothing():
    script = [(0.1, _T(0.01)), (0.1, _T(0.9)), (0.1, _T(0.01)), (0.1, _T(0.01))]
    out, p = run_policy(script)
    assert out[1] == dict(reference=-1, registered=1, accepted=0, is_reference=0)
    assert p.graph == [-1, 0, 2, 3]                       # the dropped reading is not in the graph
    assert [r["is_reference"] for r in out] == [0, 0, 0, 1]  # and does not count towards F = 3
    assert abs(p.initT[0, 3] - 0.03) < 1e-6               # nor does its correction enter initialT_
    # a gated reading is never dropped, whatever a correction would have been
    out, p = run_policy([(0.9, _T(5.0))])
    assert out[0]["accepted"] == 1 and out[0]["is_reference"] == 1 and np.array_equal(p.initT, np.eye(4))


def test_policy_gate_fires_on_nan_and_at_the_threshold():
    out, _ = run_policy([(float("nan"), _T()), (0.5, _T()), (np.nextafter(0.5, 1.0), _T())])
    assert [r["registered"] for r in out] == [0, 1, 0]
    assert sr.gate(np.array([np.nan, 0.5, 0.4, 0.6]), 0.5).tolist() == [True, False, False, True]
    # threshold 1.0 never gates a finite risk; threshold 0.0 gates every positive one
    assert not sr.gate(np.array([0.0, 0.999, 1.0]), 1.0).any()
    assert sr.gate(np.array([1e-300, 0.5, 1.0]), 0.0).all()


def test_corrected_pose_keeps_translation_and_yaw():
    """removePitchRollCorrection on a correction with a small roll: the corrected pose keeps
    corrected_origin's translation and the yaw, and takes roll and pitch from the odometry."""
    yaw, roll = np.deg2rad(20.0), np.deg2rad(2.0)
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = (Rz @ Rx).astype(np.float32)
    T[:3, 3] = [0.1, -0.2, 0.05]
    prior = np.eye(4)
    prior[:3, 3] = [1.0, 2.0, 0.7]
    moved = sr.moved_pose(T, prior)
    np.testing.assert_allclose(moved[:3, :3], Rz @ Rx, atol=1e-6)
    np.testing.assert_allclose(moved[:3, 3], (Rz @ Rx) @ prior[:3, 3] + T[:3, 3].astype(np.float64), atol=1e-6)
    fixed = sr.fix_pitch_roll(moved, prior)
    assert np.array_equal(fixed[:3, 3], moved[:3, 3])
    np.testing.assert_allclose(fixed[:3, :3], Rz, atol=1e-6)
    # a yaw-only pose comes back as itself up to the rounding of the Euler round trip
    P = np.eye(4)
    P[:3, :3] = Rz
    np.testing.assert_allclose(sr.fix_pitch_roll(P, P), P, atol=1e-15)
