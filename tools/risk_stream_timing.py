#!/usr/bin/env python3
"""Wall time of App's frame-to-reference stream with the risk gate (aicp_hip_sequence_run_risk) on
the raw C2 stream, beside the hand composition it replaces: per reading aicp_hip_prefilter,
aicp_hip_overlap, aicp_hip_alignment_features, the numpy classifier and policy of
tests/svm_reference.py, and aicp_hip_align_batch. The two alternate in one process; medians of warmed
runs; wall time around a synchronising call (both end in one). Results are checked equal first.

  python tools/risk_stream_timing.py --readings 64 --runs 5 --threshold 0.5 1.0 --out profiles/risk_stream_timing.json
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
import svm_reference as sr  # noqa: E402  (the numpy classifier, the policy, App's corrected pose)

RES = float(np.float32(0.2))


def yaw_pose(deg, t):
    a = np.deg2rad(deg)
    P = np.eye(4)
    P[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P[:3, 3] = t
    return P


def apply4(T, P):
    T, P = np.asarray(T, np.float32), np.asarray(P, np.float32)
    out = np.empty_like(P)
    for r in range(3):
        s = T[r, 0] * P[:, 0]
        s = s + T[r, 1] * P[:, 1]
        s = s + T[r, 2] * P[:, 2]
        out[:, r] = s + T[r, 3]
    return out


def compose(ctx, st, first_pose, poses, ref_model, thr, freq, rp):
    ref = ctx.prefilter(st.first)
    ref_pose = sr.fix_pitch_roll(first_pose, first_pose)
    policy = sr.GatePolicy(freq, 1.0, thr)
    Ts, flags = [], []
    for i, odom in enumerate(poses):
        rd = ctx.prefilter(st.readings[i])
        ov = ctx.overlap(ref, rd, ref_pose[:3, 3], odom[:3, 3], RES)
        feats = ctx.alignment_features(ref, rd, ref_pose, odom, rp)
        _, risk, _ = sr.predict(ref_model, np.array([[ov, feats["alignability"]]], np.float32))
        T = np.eye(4, dtype=np.float32)
        if not policy.gated(risk[0]):
            T = ctx.align_batch([dict(ref=ref, read=rd, ref_origin=ref_pose[:3, 3], read_origin=odom[:3, 3])],
                                flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP, resolution=RES)[0][0]
        d = policy.step(i, risk[0], T)
        if not d["registered"]:
            ref, ref_pose = rd, sr.fix_pitch_roll(odom, odom)
        elif d["accepted"] and d["is_reference"]:
            ref, ref_pose = apply4(T, rd), sr.fix_pitch_roll(sr.moved_pose(T, odom), odom)
        Ts.append(T)
        flags.append((d["registered"], d["accepted"], d["is_reference"], d["reference"]))
    return np.stack(Ts), flags


def measure(ctx, st, first_pose, poses, model, ref_model, thr, freq, rp, prm, runs):
    n = len(poses)

    def stream():
        return ctx.sequence_run_risk(model, thr, st.first, first_pose, st.readings, poses, params=prm, risk_params=rp)

    T, res, rec, done, rc = stream()                      # warm-up, and the equality check
    Tc, flags = compose(ctx, st, first_pose, poses, ref_model, thr, freq, rp)
    assert rc == 0 and done == n
    assert T.tobytes() == Tc.tobytes(), "stream and composition differ"
    assert flags == [(q["registered"], r["accepted"], r["is_reference"], r["reference"]) for r, q in zip(res, rec)]
    t_stream, t_comp = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        stream()
        t1 = time.perf_counter()
        compose(ctx, st, first_pose, poses, ref_model, thr, freq, rp)
        t2 = time.perf_counter()
        t_stream.append((t1 - t0) * 1e3)
        t_comp.append((t2 - t1) * 1e3)
    return dict(threshold=thr, gated=int(sum(1 - q["registered"] for q in rec)),
                dropped=int(sum(q["registered"] and not r["accepted"] for r, q in zip(res, rec))),
                references=int(sum(r["is_reference"] for r in res)),
                stream_ms_median=float(np.median(t_stream)), stream_ms_min=min(t_stream), stream_ms_max=max(t_stream),
                composition_ms_median=float(np.median(t_comp)), composition_ms_min=min(t_comp),
                composition_ms_max=max(t_comp), stream_ms_per_reading=float(np.median(t_stream)) / n,
                composition_ms_per_reading=float(np.median(t_comp)) / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threshold", type=float, nargs="+", default=[0.5, 1.0],
                    help="one measurement per threshold (the golden model's risks lie near 0.5: 1.0 gates nothing)")
    ap.add_argument("--model", default=os.path.join(sr.GOLDEN, sr.MODELS["opencv3"][0]))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = sy.make_stream(n_readings=a.readings, n_points=a.points, seed=1)
    first_pose = yaw_pose(0.0, st.first_origin)
    poses = [yaw_pose(1.0 * (i + 1), st.origins[i]) for i in range(a.readings)]
    ctx = L.Context(0)
    model, ref_model = L.SvmModel(a.model), sr.read_model(a.model)
    rp = L.default_risk_params(angular_view=270.0)
    prm = L.default_sequence_params(max_correction_magnitude=1.0, resolution=RES, flags=L.AICP_RUN_OVERLAP)
    freq = prm.reference_update_frequency

    cases = []
    for thr in a.threshold:
        cases.append(measure(ctx, st, first_pose, poses, model, ref_model, thr, freq, rp, prm, a.runs))
    out = dict(readings=a.readings, points=a.points, runs=a.runs, model=os.path.basename(a.model), cases=cases,
               library=L.provenance())
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
