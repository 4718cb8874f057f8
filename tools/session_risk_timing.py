#!/usr/bin/env python3
"""Per-reading time of failure_prediction_mode served live (AppSession(..., risk=...), one reading
per call on the resident buffers) against aicp_hip_sequence_run_risk on the same recording: the raw
C2 stream, the golden opencv3 model, thresholds 0.5 and 1.0, robot and debug mode. The "baseline",
aicp_hip_sequence_run_risk, is the same reading step driven from C on a session private to the call,
so the comparison shows the overhead of calling reading by reading from Python and nothing else
(profiles/session_risk_timing.json records it when it was a host loop of its own; the `baseline`
list of copies_of_the_median_reading describes that loop). One process, one
device; the two variants alternate inside every round; one warm-up round, then medians of the rounds
with (min, max); wall time around synchronising calls. Results are compared for bit equality before
anything is timed.

Also reported: the session's device time per reading (HIP events, origin upload to the last kernel),
the per-phase aicp_risk_stats of its features (median over the readings of the last round), and the
host<->device copies of one call by size, listed from the code paths for the median reading (they
are not traced).

  python tools/session_risk_timing.py --out profiles/session_risk_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aicp_mapping_amd._lib as L  # noqa: E402
from aicp_mapping_amd import synthetic as sy  # noqa: E402
from aicp_mapping_amd.session import AppSession  # noqa: E402
import svm_reference as sr  # noqa: E402  (the golden model's path)

RES = float(np.float32(0.2))
PHASES = ("fov_ms", "prefilter_a_ms", "prefilter_b_ms", "clusters_ms", "counts_ms", "match_ms", "device_ms", "wall_ms")


def yaw_pose(deg, t):
    a = np.deg2rad(deg)
    P = np.eye(4)
    P[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P[:3, 3] = t
    return P


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def copies(n_raw, stride, n_ref, kept, gated):
    """One call's host<->device copies by size (bytes), from the code paths."""
    session = [("H2D", n_raw * stride, "the reading's raw rows (0 from a sweep accumulator)"),
               ("H2D", 24, "prior origin"),
               ("D2H", "3 x small", "pre-filter control blocks (reading, FOV-kept reference, FOV-kept reading)"),
               ("H2D", "descriptors + block maps", "overlap-only batch (no points)"),
               ("D2H", "state + descriptor", "overlap-only batch"),
               ("D2H", 8, "FOV kept counts"),
               ("D2H", "cluster matches", "risk_core's result"),
               ("D2H", 352, "state | record | header | origin | gate record")]
    if not gated:
        session += [("H2D", "descriptors + block maps", "ICP-only batch (no points)"),
                    ("D2H", "state + 64 + descriptor", "ICP-only batch"),
                    ("D2H", 256, "state | record | header")]
    base = [("H2D", n_raw * stride, "the reading's raw rows"),
            ("D2H", kept * 16, "the kept points (pf_cloud)"),
            ("H2D", kept * 16, "overlap batch: the reading (the reference too when it is new: %d)" % (n_ref * 16)),
            ("H2D", (n_ref + kept) * 16, "alignment_features: both clouds"),
            ("D2H", 32, "gate record")]
    if not gated:
        base += [("H2D", 0, "ICP batch: the reading and the reference are resident from the overlap batch's caches"
                  " when unchanged, else %d" % ((n_ref + kept) * 16))]
    return dict(session=session, baseline=base)


def measure(ctx, st, first_pose, poses, model, thr, debug, rp, rounds):
    n = len(poses)
    prm = L.default_sequence_params(max_correction_magnitude=1.0, resolution=RES,
                                    flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))
    s = AppSession(ctx, params=prm, prefilter=True, risk=dict(model=model, threshold=thr, params=rp))

    def baseline():
        return ctx.sequence_run_risk(model, thr, st.first, first_pose, st.readings, poses, params=prm, risk_params=rp)

    def session(collect=None):
        s.start(st.first, pose=first_pose)
        out = []
        for i in range(n):
            t0 = time.perf_counter()
            r = s.process(st.readings[i], pose=poses[i])
            t1 = time.perf_counter()
            out.append(r)
            if collect is not None:
                collect["wall"].append((t1 - t0) * 1e3)
                collect["device"].append(s.last_timing()["device_ms"])
                collect["risk"].append(ctx.last_risk_stats())
        return out

    # warm-up round, and the equality check
    T, res, rec, done, rc = baseline()
    got = session()
    assert rc == 0 and done == n
    for i, (Ti, ri, ki, qi) in enumerate(got):
        assert Ti.tobytes() == T[i].tobytes(), ("T", i)
        assert {k: v for k, v in ri.items() if k != "rc"} == res[i], ("result", i)
        assert all(np.asarray(qi[k]).tobytes() == np.asarray(rec[i][k]).tobytes() for k in qi), ("record", i)
    t_base, t_sess, per = [], [], None
    for _ in range(rounds):
        t0 = time.perf_counter()
        baseline()
        t1 = time.perf_counter()
        per = dict(wall=[], device=[], risk=[])
        session(per)
        t2 = time.perf_counter()
        t_base.append((t1 - t0) * 1e3 / n)
        t_sess.append((t2 - t1) * 1e3 / n)
    s.close()
    kept = [q["n_read"] for q in rec]
    med = int(np.argsort(kept)[len(kept) // 2])
    gated = [1 - q["registered"] for q in rec]
    return dict(threshold=thr, mode="debug" if debug else "robot", gated=int(sum(gated)),
                dropped=int(sum(q["registered"] and not r["accepted"] for r, q in zip(res, rec))),
                references=int(sum(r["is_reference"] for r in res)),
                baseline_ms_per_reading=stats(t_base), session_ms_per_reading=stats(t_sess),
                session_call_wall_ms=stats(per["wall"]), session_call_device_ms=stats(per["device"]),
                session_risk_stats_ms={k: float(np.median([r[k] for r in per["risk"]])) for k in PHASES},
                copies_of_the_median_reading=copies(len(st.readings[med]), 12, kept[med - 1] if med else kept[med],
                                                    kept[med], bool(gated[med])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--model", default=os.path.join(sr.GOLDEN, sr.MODELS["opencv3"][0]))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = sy.make_stream(n_readings=a.readings, n_points=a.points, seed=1)
    first_pose = yaw_pose(0.0, st.first_origin)
    poses = [yaw_pose(1.0 * (i + 1), st.origins[i]) for i in range(a.readings)]
    ctx = L.Context(0)
    model = L.SvmModel(a.model)
    rp = L.default_risk_params(angular_view=270.0)
    cases = []
    for thr in a.threshold:
        for debug in (False, True):
            c = measure(ctx, st, first_pose, poses, model, thr, debug, rp, a.rounds)
            cases.append(c)
            print(json.dumps({k: c[k] for k in ("threshold", "mode", "gated", "baseline_ms_per_reading",
                                                "session_ms_per_reading", "session_call_device_ms")}), flush=True)
    out = dict(readings=a.readings, points=a.points, frequency=5, view=270.0, rounds=a.rounds, warmup_rounds=1,
               model=os.path.basename(a.model), cases=cases, library=L.provenance())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
