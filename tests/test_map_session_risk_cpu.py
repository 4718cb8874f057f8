"""CPU checks for the live map sessions with failure_prediction_mode (aicp_hip_mapsession_create_risk
and the _risk calls): the new entry points are declared in the header and bound in _lib.py, null
arguments are refused, and MapGatePolicy (tests/map_session_risk_reference.py), the bookkeeping the
GPU tests compare the sessions' state with, takes the decisions of include/aicp_hip.h on
hand-written sequences: both policies, the gated branch's map rules, debug mode's initialT_."""
import ctypes as C
import os
import re

import numpy as np

import map_session_risk_reference as mr
import svm_reference as sr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aicp_hip_mapsession_create_risk", "aicp_hip_mapsession_process_risk",
       "aicp_hip_mapsession_process_accum_risk"]
GATE, PASS = 0.9, 0.1  # risks on either side of the threshold 0.5


def shift(x, y=0.0, z=0.0):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = [x, y, z]
    return T


def walk(policy, steps):
    """steps: (risk, x shift) per reading -> (registered, accepted, append, refilter, count) per reading."""
    out = []
    for risk, x in steps:
        d = policy.step(risk, shift(x))
        out.append((d["registered"], d["accepted"], d["append"], d["refilter"], policy.count))
    return out


def test_new_symbols_are_declared_and_bound():
    import aicp_mapping_amd._lib as L

    header = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.EXPORTS and name in L._NEWEST, name
        assert getattr(L.lib, name).argtypes is not None, name
    assert len(L.lib.aicp_hip_mapsession_create_risk.argtypes) == 10
    assert len(L.lib.aicp_hip_mapsession_process_risk.argtypes) == 8
    assert len(L.lib.aicp_hip_mapsession_process_accum_risk.argtypes) == 8
    # the aicp_hip_map_session_* family stays the seven names tests/test_map_session_cpu.py pins
    assert len(set(re.findall(r"\b(aicp_hip_map_session_\w+)\s*\(", header))) == 7
    from aicp_mapping_amd.map_session import MapSession

    assert {"risk"} <= set(MapSession.__init__.__code__.co_varnames)


def test_null_arguments_are_refused():
    import aicp_mapping_amd._lib as L

    lib, bad = L.lib, L.AICP_ERR_INVALID
    cfg, loc, rp = L.default_config(), L.default_localization_params(), L.default_risk_params()
    h = C.c_void_p()
    assert lib.aicp_hip_mapsession_create_risk(None, C.byref(cfg), C.byref(loc), None, None, None, C.byref(rp), None,
                                               0.5, C.byref(h)) == bad
    assert lib.aicp_hip_mapsession_create_risk(None, C.byref(cfg), C.byref(loc), None, None, None, C.byref(rp), None,
                                               0.5, None) == bad
    pts = np.zeros((4, 3), F32)
    c, keep = L.make_cloud(pts)
    pose = np.eye(4).reshape(16)
    T = np.zeros(16, F32)
    res, rec, kept = L.LocalizationResult(), L.PipelineRecord(), C.c_uint32()
    assert lib.aicp_hip_mapsession_process_risk(None, None, C.byref(c), L._dptr(pose), L._fptr(T), C.byref(res),
                                                C.byref(rec), C.byref(kept)) == bad
    assert lib.aicp_hip_mapsession_process_accum_risk(None, None, None, L._dptr(pose), L._fptr(T), C.byref(res),
                                                      C.byref(rec), C.byref(kept)) == bad


def test_prior_map_a_gated_first_reading_refilters_and_does_not_merge():
    p = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=4)
    assert walk(p, [(GATE, 9.0)]) == [(0, 1, 0, 1, 1)]
    # an ungated first reading merges and re-filters
    q = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=4)
    assert walk(q, [(PASS, 0.1)]) == [(1, 1, 1, 1, 1)]
    # merging off: neither, and the count still moves
    r = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=4, merge=False)
    assert walk(r, [(GATE, 0.0), (PASS, 0.1)]) == [(0, 1, 0, 0, 1), (1, 1, 0, 0, 2)]


def test_prior_map_a_gated_reading_at_a_merge_slot_does_not_merge():
    """frequency 3, re-filter every 4: the clouds 1, 4, 7 of the graph are merge slots, 1, 5, 9 re-filter."""
    p = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=4)
    got = walk(p, [(PASS, 0.1), (PASS, 0.1), (PASS, 0.1), (GATE, 0.0), (GATE, 0.0), (PASS, 0.1), (PASS, 0.1)])
    assert got == [(1, 1, 1, 1, 1), (1, 1, 0, 0, 2), (1, 1, 0, 0, 3),
                   (0, 1, 0, 0, 4),   # cloud 4: a merge slot, gated: no merge
                   (0, 1, 0, 1, 5),   # cloud 5: gated, the re-filter still applies
                   (1, 1, 0, 0, 6), (1, 1, 1, 0, 7)]
    # a NaN risk gates: !(risk <= threshold)
    assert walk(p, [(float("nan"), 0.0)]) == [(0, 1, 0, 0, 8)]


def test_prior_map_the_first_reading_drop_exemption_ends_after_a_gated_first_reading():
    big = 0.6  # above max_correction_magnitude 0.5
    p = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=0)
    assert walk(p, [(PASS, big), (PASS, big)]) == [(1, 1, 1, 0, 1), (1, 0, 0, 0, 1)]  # the first is never dropped
    q = mr.MapGatePolicy(False, 3, 0.5, 0.5, refilter_every=0)
    assert walk(q, [(GATE, 0.0), (PASS, big), (PASS, 0.1)]) == [(0, 1, 0, 0, 1), (1, 0, 0, 0, 1), (1, 1, 0, 0, 2)]
    # a gated reading itself is never dropped, whatever its correction would have been
    assert walk(q, [(GATE, 9.0)]) == [(0, 1, 0, 0, 3)]


def test_built_map_a_gate_resets_the_count_in_mid_window_and_appends():
    p = mr.MapGatePolicy(True, 3, 0.5, 0.5)
    got = walk(p, [(PASS, 0.1), (PASS, 0.1), (GATE, 9.0), (PASS, 0.1), (PASS, 0.6), (PASS, 0.1), (PASS, 0.1),
                   (GATE, 0.0), (GATE, 0.0)])
    assert got == [(1, 1, 0, 0, 1), (1, 1, 0, 0, 2),
                   (0, 1, 1, 0, 0),                   # gated at acc 2: appended, the count restarts
                   (1, 1, 0, 0, 1), (1, 0, 0, 0, 1),  # the drop test applies to the first reading too
                   (1, 1, 0, 0, 2), (1, 1, 1, 0, 0),  # the third accepted since the gate is the reference
                   (0, 1, 1, 0, 0), (0, 1, 1, 0, 0)]
    # at the threshold the reading is registered
    assert walk(mr.MapGatePolicy(True, 3, 0.5, 0.5), [(0.5, 0.1)]) == [(1, 1, 0, 0, 1)]


def test_debug_mode_initial_T_is_unchanged_by_a_gate():
    for built in (False, True):
        p = mr.MapGatePolicy(built, 2, 0.5, 0.5, refilter_every=3)
        p.step(PASS, shift(0.1))
        I1 = p.initT.copy()
        assert I1.tobytes() == sr.mul4f(shift(0.1), np.eye(4, dtype=F32)).tobytes()
        p.step(GATE, shift(9.0))
        assert p.initT.tobytes() == I1.tobytes()
        p.step(PASS, shift(0.6))  # dropped: unchanged too
        assert p.initT.tobytes() == I1.tobytes()
        p.step(PASS, shift(-0.2))
        assert p.initT.tobytes() == sr.mul4f(shift(-0.2), I1).tobytes()
