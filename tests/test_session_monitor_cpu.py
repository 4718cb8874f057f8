"""The quality monitor per reading in the live sessions, the CPU side: the header declares the new
entry points and the library exports them, the argument checks that need no device refuse what they
should, the Python monitor= argument is handled before anything is made, and the raw fixture on
which tests/test_session_monitor.py compares the sessions has what those comparisons rely on: the
replay of App (tests/session_reference.py on the oracle) drops reading 3 and promotes reading 5
(frequency 5, both modes) or readings 2 and 6 (frequency 3, robot mode)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import session_reference as sr
from aicp_mapping_amd import synthetic as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aicp_hip_session_set_monitor", "aicp_hip_session_last_monitor", "aicp_hip_session_monitor_counters",
       "aicp_hip_mapsession_set_monitor", "aicp_hip_mapsession_last_monitor", "aicp_hip_mapsession_monitor_counters",
       "aicp_hip_test_monitor_resident")


def test_header_declares_and_library_exports_the_new_symbols():
    import aicp_mapping_amd._lib as L

    txt = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    so = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in L.EXPORTS and hasattr(so, name), name
        assert getattr(L.lib, name).argtypes, name
    for kind in ("session", "mapsession"):
        assert len(getattr(L.lib, f"aicp_hip_{kind}_set_monitor").argtypes) == 3
        assert len(getattr(L.lib, f"aicp_hip_{kind}_last_monitor").argtypes) == 3
        assert len(getattr(L.lib, f"aicp_hip_{kind}_monitor_counters").argtypes) == 2
    assert C.sizeof(L.MonitorResult) == 56


def test_null_arguments_need_no_device():
    import aicp_mapping_amd._lib as L

    lib, bad = L.lib, L.AICP_ERR_INVALID
    prm, res, valid, cnt = L.default_monitor_params(), L.MonitorResult(), C.c_int32(7), (C.c_uint64 * 4)(1, 2, 3, 4)
    for kind in ("session", "mapsession"):
        assert getattr(lib, f"aicp_hip_{kind}_set_monitor")(None, None, C.byref(prm)) == bad
        assert getattr(lib, f"aicp_hip_{kind}_set_monitor")(None, None, None) == bad
        assert getattr(lib, f"aicp_hip_{kind}_last_monitor")(None, C.byref(res), C.byref(valid)) == bad
        assert getattr(lib, f"aicp_hip_{kind}_monitor_counters")(None, cnt) == bad
    assert valid.value == 7 and list(cnt) == [1, 2, 3, 4]
    pts, T = np.zeros((4, 3), np.float32), np.eye(4, dtype=np.float32).reshape(16)
    dirty = C.c_uint64(5)
    assert lib.aicp_hip_test_monitor_resident(None, C.byref(prm), None, L._fptr(pts), 4, L._fptr(pts), 4, L._fptr(T), 1,
                                              C.byref(res), C.byref(dirty), cnt) == bad
    assert dirty.value == 5


def test_python_monitor_argument():
    import aicp_mapping_amd._lib as L
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.session import AppSession

    assert L.monitor_argument(None) is None and L.monitor_argument(False) is None
    d = L.monitor_argument(True)
    assert (d.quantile, d.max_accepted_dist, d.flags) == (np.float32(0.6), 0.2, 0)
    p = L.monitor_argument(dict(quantile=0.5, max_accepted_dist=0.1, paired=True))
    assert (p.quantile, p.max_accepted_dist, p.flags) == (0.5, 0.1, L.AICP_MON_PAIRED)
    assert L.monitor_argument(dict(paired=False)).flags == 0
    mine = L.default_monitor_params(quantile=0.25)
    copy = L.monitor_argument(mine)
    assert copy is not mine and bytes(copy) == bytes(mine)
    with pytest.raises(ValueError):
        L.monitor_argument(dict(quantil=0.5))
    with pytest.raises(TypeError):
        L.monitor_argument(0.6)
    # the sessions check the argument before they make anything (a context is not even looked at)
    with pytest.raises(ValueError):
        AppSession(None, monitor=dict(bucket=4))
    with pytest.raises(TypeError):
        MapSession(None, None, monitor="on")
    for cls in (AppSession, MapSession):
        for m in ("set_monitor", "last_monitor", "monitor_counters"):
            assert callable(getattr(cls, m)), (cls, m)
    assert AppSession._monitor_kind == "session" and MapSession._monitor_kind == "mapsession"
    assert L.MONITOR_COUNTERS == ("readings", "trees", "reference_reuses", "chain_trees")


@pytest.mark.parametrize("debug,freq,promoted", [(False, 5, [5]), (True, 5, [5]), (False, 3, [2, 6])],
                         ids=["robot-5", "debug-5", "robot-3"])
def test_the_raw_fixture_drops_reading_3_and_promotes(oracle, freq, promoted, debug):
    """What tests/test_session_monitor.py's counters and old-reference comparisons rely on in its
    three cases, from the oracle alone: 9 registered readings, reading 3 dropped by
    max_correction_magnitude 0.4, the promotions, and a registered reading per record."""
    st = sy.make_stream(n_readings=9, n_points=20000, seed=8, half=12.0, jumps={3: (0, -0.8, 0)})
    loop, end = sr.replay(sr.OracleBackend(oracle, resolution=float(np.float32(0.2))), oracle, st.first,
                          st.first_origin, st.readings, st.origins, freq=freq, max_corr=0.4, debug=debug, raw=True)
    assert len(loop) == 9 and not end["ended"]
    assert [r["status"] for r in loop] == [0] * 9
    assert [r["accepted"] for r in loop] == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert [i for i, r in enumerate(loop) if r["is_reference"]] == promoted
    assert len({r["reference"] for r in loop}) == 1 + len([p for p in promoted if p < 8])
    assert all(len(r["registered"]) == r["n_kept"] > 0 for r in loop)
