"""CPU checks for the live session with failure_prediction_mode: the host loop the GPU tests compare
the session's state with (tests/session_risk_reference.py) takes svm_reference.GatePolicy's
decisions and keeps App's reference, pose and initialT_ on a scripted sequence with stand-in
building blocks; the new entry points are declared in the header and bound in _lib.py."""
import os
import re

import numpy as np

import session_risk_reference as srr
import svm_reference as sr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aicp_hip_session_create_risk", "aicp_hip_session_start_pose", "aicp_hip_session_start_accum_pose",
       "aicp_hip_session_process_risk", "aicp_hip_session_process_accum_risk", "aicp_hip_session_reference_pose"]


def shift(x, y=0.0, z=0.0):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = [x, y, z]
    return T


class Script:
    """Stand-in blocks: reading i has risk risks[i] and correction Ts[i]; clouds pass unfiltered."""

    def __init__(self, risks, Ts):
        self.risks, self.Ts, self.i, self.registered, self.moved_by = risks, Ts, -1, [], []

    def prefilter(self, cloud):
        return np.ascontiguousarray(cloud, F32)

    def transform(self, T, cloud):
        self.moved_by.append(np.asarray(T, F32).copy())
        return srr.apply4(T, cloud)

    def overlap(self, ref, read, o_ref, o_read):
        self.i += 1
        return 50.0

    def alignability(self, ref, read, ref_pose, read_pose):
        return 0.5

    def risk(self, overlap, alignability):
        return self.risks[self.i]

    def register(self, ref, read, o_ref, o_read):
        self.registered.append(self.i)
        return self.Ts[self.i], 7


#          0 accepted   1 dropped    2 promoted (F = 2)  3 gated  4 accepted  5 at the threshold: registered, promoted
RISKS = [0.1, 0.2, 0.3, 0.9, 0.0, 0.5, float("nan")]     # 6: a NaN risk is gated (!(risk <= threshold))
SHIFTS = [0.1, 0.6, -0.2, 9.0, 0.05, 0.0, 9.0]
EXPECT = [  # reference, registered, accepted, is_reference
    (-1, 1, 1, 0), (-1, 1, 0, 0), (-1, 1, 1, 1), (2, 0, 1, 1), (3, 1, 1, 0), (3, 1, 1, 1), (5, 0, 1, 1)]


def run(debug):
    rng = np.random.default_rng(3)
    first = rng.uniform(-5, 5, (40, 3)).astype(F32)
    readings = [rng.uniform(-5, 5, (30 + i, 3)).astype(F32) for i in range(len(RISKS))]
    poses = [np.eye(4) for _ in RISKS]
    for i, P in enumerate(poses):
        P[:3, 3] = [0.3 * (i + 1), 0.0, 0.7]
    blocks = Script(RISKS, [shift(s) for s in SHIFTS])
    out = srr.host_loop(blocks, first, np.eye(4), readings, poses, freq=2, max_corr=0.5, threshold=0.5, debug=debug)
    return first, readings, poses, blocks, out


def test_the_loop_takes_the_policys_decisions():
    for debug in (False, True):
        first, readings, poses, blocks, out = run(debug)
        policy = sr.GatePolicy(2, 0.5, 0.5)
        for i, (d, e) in enumerate(zip(out, EXPECT)):
            want = policy.step(i, RISKS[i], shift(SHIFTS[i]))
            got = {k: d[k] for k in ("reference", "registered", "accepted", "is_reference")}
            assert got == want, (debug, i)
            assert tuple(got.values()) == e, (debug, i)
            assert d["initial_T"].tobytes() == policy.initT.tobytes(), (debug, i)
        assert blocks.registered == [0, 1, 2, 4, 5]           # a gated reading is not registered
        assert out[3]["iterations"] == 0 and np.array_equal(out[3]["T"], np.eye(4, dtype=F32))
        assert out[1]["corrected_origin"] is None              # dropped
        # initialT_: the accepted corrections only (0.1 - 0.2 + 0.05 + 0.0), the dropped and gated ones left out
        assert abs(float(out[-1]["initial_T"][0, 3]) - (-0.05)) < 1e-6


def test_the_loop_keeps_the_reference_and_its_pose():
    first, readings, poses, blocks, out = run(False)
    assert out[0]["ref"].tobytes() == first.tobytes() and out[1]["ref"].tobytes() == first.tobytes()
    assert out[1]["ref_pose"].tobytes() == out[0]["ref_pose"].tobytes() == sr.fix_pitch_roll(np.eye(4), np.eye(4)).tobytes()
    # promoted: the reading moved by its correction; its pose fix_pitch_roll(moved_pose(T, prior), odom)
    assert out[2]["ref"].tobytes() == srr.apply4(shift(-0.2), readings[2]).tobytes()
    want = sr.fix_pitch_roll(sr.moved_pose(shift(-0.2), poses[2]), poses[2])
    assert out[2]["ref_pose"].tobytes() == want.tobytes()
    assert np.array_equal(out[2]["corrected_origin"], sr.moved_pose(shift(-0.2), poses[2])[:3, 3])
    # gated: the reading's own bytes; its pose fix_pitch_roll(prior, odom); corrected_origin the prior's translation
    assert out[3]["ref"].tobytes() == readings[3].tobytes()
    assert out[3]["ref_pose"].tobytes() == sr.fix_pitch_roll(poses[3], poses[3]).tobytes()
    assert np.array_equal(out[3]["corrected_origin"], poses[3][:3, 3])
    assert out[4]["ref"].tobytes() == readings[3].tobytes()


def test_debug_mode_moves_the_reading_and_its_pose_by_initial_T():
    first, readings, poses, blocks, out = run(True)
    assert len(blocks.moved_by) == len(RISKS)
    assert np.array_equal(blocks.moved_by[0], np.eye(4, dtype=F32))
    for i in range(1, len(RISKS)):
        assert blocks.moved_by[i].tobytes() == out[i - 1]["initial_T"].tobytes(), i
    # the gated reading 3 is the reference as it was moved, with the moved prior pose
    I3 = out[2]["initial_T"]
    assert out[3]["ref"].tobytes() == srr.apply4(I3, readings[3]).tobytes()
    prior = sr.moved_pose(I3, poses[3])
    assert np.array_equal(out[3]["corrected_origin"], prior[:3, 3])
    assert out[3]["ref_pose"].tobytes() == sr.fix_pitch_roll(prior, poses[3]).tobytes()
    assert out[3]["initial_T"].tobytes() == I3.tobytes()    # a gated reading leaves initialT_


def test_new_symbols_are_declared_and_bound():
    import aicp_mapping_amd._lib as L

    header = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.EXPORTS and name in L._NEWEST, name
        fn = getattr(L.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) >= 3, name
    assert len(L.lib.aicp_hip_session_create_risk.argtypes) == 8
    assert len(L.lib.aicp_hip_session_process_risk.argtypes) == 8
    assert len(L.lib.aicp_hip_session_process_accum_risk.argtypes) == 8
    from aicp_mapping_amd.session import AppSession

    assert {"risk"} <= set(AppSession.__init__.__code__.co_varnames)
    assert hasattr(AppSession, "reference_pose")
