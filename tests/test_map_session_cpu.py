"""The live map sessions (aicp_hip_map_session_*), the CPU side: the C ABI and its Python bindings
are there, the argument checks that need no device refuse what they should, and the frequency-1
variant of the raw fixtures, on which tests/test_map_session.py compares a session with the
robot-mode stream bit for bit, has something to decide: the replay alone drops, merges and
re-filters on it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import built_map_reference as bm
import localization_reference as lr
import raw_stream_reference as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aicp_hip_map_session_create", "aicp_hip_map_session_free", "aicp_hip_map_session_start",
       "aicp_hip_map_session_process", "aicp_hip_map_session_process_accum", "aicp_hip_map_session_state",
       "aicp_hip_map_session_last_timing")
# what the bit-for-bit robot-mode comparison of tests/test_map_session.py runs at (every window of
# the stream is one reading long); the other PARAMS stay
FREQ1 = dict(reference_update_frequency=1)


def test_header_declares_and_library_exports_the_new_symbols():
    import aicp_mapping_amd._lib as L

    txt = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(aicp_hip_map_session_\w+)\s*\(", txt))
    assert declared == set(NEW)
    for name in NEW:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, txt), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes, name
    # the stream's arguments without the recording, plus the reading's pose and kept
    assert len(L.lib.aicp_hip_map_session_process.argtypes) == len(L.lib.aicp_hip_map_session_process_accum.argtypes)


def test_python_exports_the_session():
    import aicp_mapping_amd as pkg
    from aicp_mapping_amd.map_session import MapSession

    assert pkg.MapSession is MapSession and "MapSession" in pkg.__all__
    for m in ("start", "process", "state", "last_timing", "close"):
        assert callable(getattr(MapSession, m)), m


def test_null_arguments_need_no_device():
    """Every entry point refuses a NULL context or session before it touches the device. (What
    create refuses of its parameters needs a context: tests/test_map_session.py.)"""
    import aicp_mapping_amd._lib as L

    lib, bad = L.lib, L.AICP_ERR_INVALID
    cfg, loc, bmp = L.default_config(), L.default_localization_params(), L.default_built_map_params()
    h = C.c_void_p(77)
    assert lib.aicp_hip_map_session_create(None, C.byref(cfg), C.byref(loc), None, None, None, C.byref(h)) == bad
    assert h.value == 77
    assert lib.aicp_hip_map_session_create(None, C.byref(cfg), None, C.byref(bmp), None, None, None) == bad
    lib.aicp_hip_map_session_free(None, None)
    assert lib.aicp_hip_map_session_start(None, None, None) == bad
    T, pose = np.zeros(16, np.float32), np.eye(4, dtype=np.float32).reshape(16)
    res, kept = L.LocalizationResult(), C.c_uint32(9)
    c, keep = L.make_cloud(np.zeros((4, 3), np.float32), (0, 0, 0))
    assert lib.aicp_hip_map_session_process(None, None, C.byref(c), L._fptr(pose), L._fptr(T), C.byref(res),
                                            C.byref(kept)) == bad
    assert lib.aicp_hip_map_session_process_accum(None, None, None, L._fptr(pose), L._fptr(T), C.byref(res),
                                                  C.byref(kept)) == bad
    assert kept.value == 9 and res.status == 0
    assert lib.aicp_hip_map_session_state(None, None, None, None, None, None) == bad
    assert lib.aicp_hip_map_session_last_timing(None, None, None) == bad


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_the_prior_fixture_at_frequency_1_has_something_to_decide(oracle, debug):
    mp, raws, poses, origins = rs.prior_world(oracle)
    rec, final = rs.replay_prior_raw(oracle, mp, raws, poses, origins, debug=debug, **dict(lr.PARAMS, **FREQ1))
    assert [r["status"] for r in rec] == [0] * rs.N_PRIOR
    accepted = [r["accepted"] for r in rec]
    merged = [i for i, r in enumerate(rec) if r["merged"]]
    refiltered = [i for i, r in enumerate(rec) if r["refiltered"]]
    assert accepted.count(0) >= 1 and len(merged) >= 2 and len(refiltered) >= 1
    # at frequency 1 every accepted reading is merged, and the 1st and the 5th accepted (lr.PARAMS:
    # every 4th cloud after the first) re-filter the map
    assert merged == [i for i, a in enumerate(accepted) if a]
    assert accepted == [1, 1, 0, 1, 1, 0, 1, 1] and refiltered == [0, 6]


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_the_built_fixture_at_frequency_1_drops_a_reading(oracle, debug):
    first, raws, poses, origins = rs.built_world(oracle)
    rec, final = rs.replay_built_raw(oracle, first, raws, poses, origins, debug=debug, **dict(bm.PARAMS, **FREQ1))
    assert [r["status"] for r in rec] == [0] * rs.N_BUILT
    accepted = [r["accepted"] for r in rec]
    assert accepted.count(0) >= 1 and accepted.count(1) >= 2
    assert [r["is_reference"] for r in rec] == accepted  # every accepted reading is the next reference
    assert len(final) == len(first) + sum(r["kept"] for r in rec if r["is_reference"])
