"""tests/session_reference.py pinned on the CPU: its one-pair loop, with the oracle's building blocks
in place of the device calls, equals oracle.sequence (the replay of App::processCloud every stream
test is checked against) record for record, in both working modes, from raw and from pre-filtered
clouds, across a dropped reading and two reference updates."""
import numpy as np
import pytest

import session_reference as sr
from aicp_mapping_amd import synthetic as sy

RES = float(np.float32(0.2))


def _same(records, ref):
    assert len(records) == len(ref)
    for i, (a, b) in enumerate(zip(records, ref)):
        assert a["status"] == b["status"], i
        for k in ("reference", "accepted", "is_reference"):
            assert a[k] == b[k], (i, k)
        assert np.array_equal(np.asarray(a["T"], np.float32), np.asarray(b["T"], np.float32)), i
        assert a["counts"] == [int(c) for c in b["counts"]] and a["ratio"] == b["ratio"], i
        assert a["iterations"] == b["stats"].iterations, i
        assert np.array_equal(a["prior_origin"], b["prior_origin"]), i
        if b["accepted"]:
            assert np.array_equal(a["corrected_origin"], b["corrected_origin"]), i
        else:
            assert a["corrected_origin"] is None and b["corrected_origin"] is None
        if "n_kept" in b:
            assert a["n_kept"] == b["n_kept"], i


@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_loop_equals_the_oracle_stream_prefiltered(oracle, mode):
    st = sy.make_stream(n_readings=6, n_points=3000, seed=8, half=18.0, jumps={2: (0.6, 0, 0)})
    ref = oracle.sequence(st.first, st.first_origin, st.readings, st.origins, reference_update_frequency=2,
                          max_correction_magnitude=0.4, resolution=RES, working_mode=mode)
    assert [r["accepted"] for r in ref] == [1, 1, 0, 1, 1, 1] and [r["is_reference"] for r in ref] == [0, 1, 0, 0, 1, 0]
    got, state = sr.replay(sr.OracleBackend(oracle, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                           st.origins, freq=2, max_corr=0.4, debug=mode == "debug", raw=False)
    _same(got, ref)
    assert state["ref_id"] == 4 and not state["ended"]
    assert np.array_equal(state["reference"], oracle.transform_cloud(got[4]["T"], got[4]["registered"]))
    if mode == "debug":
        assert not np.array_equal(state["initT"], np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("mode", ["robot", "debug"])
def test_loop_equals_the_oracle_stream_raw(oracle, mode):
    st = sy.make_stream(n_readings=3, n_points=8000, seed=8, half=8.0)
    ref = oracle.sequence(st.first, st.first_origin, st.readings, st.origins, reference_update_frequency=2,
                          resolution=RES, working_mode=mode, prefilter_with=True)
    assert [r["is_reference"] for r in ref] == [0, 1, 0] and all(50 <= r["n_kept"] < 8000 for r in ref)
    got, state = sr.replay(sr.OracleBackend(oracle, resolution=RES), oracle, st.first, st.first_origin, st.readings,
                           st.origins, freq=2, debug=mode == "debug", raw=True)
    _same(got, ref)
    assert state["ref_id"] == 1


def test_loop_ends_at_an_emptied_reading(oracle):
    st = sy.make_stream(n_readings=3, n_points=8000, seed=8, half=8.0)
    rng = np.random.default_rng(4)
    reads = [st.readings[0], rng.uniform(-40, 40, size=(30, 3)).astype(np.float32), st.readings[2]]
    got, state = sr.replay(sr.OracleBackend(oracle, resolution=RES), oracle, st.first, st.first_origin, reads,
                           st.origins, raw=True)
    assert len(got) == 2 and got[1]["status"] == sr.ERR_INVALID and got[1]["n_kept"] == 0 and state["ended"]
    ref = oracle.sequence(st.first, st.first_origin, reads, st.origins, resolution=RES, prefilter_with=True, stop=1)
    _same(got[:1], ref)
