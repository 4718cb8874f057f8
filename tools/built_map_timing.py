"""Time App's built-map localization stream (BuiltMap.sequence_run,
aicp_hip_built_map_sequence_run) against the hand composition of the entry points that served the
mode before it: per window every crop to the host (PriorMap.crop), the crops uploaded again inside
Context.align_batch (overlap -> ratio -> ICP), the drop test and the count on the host, and every
reference reading uploaded a second time (PriorMap.merge); in debug mode the reading also goes
through Context.transform and back. The composition uses none of the new entry points, so its
time is the previous commit's.

Workload: a 120 k-point first cloud, 64 readings of 120 k points, crop -15..15, a reference every
5 accepted readings, octree 0.2 m; robot and debug working mode.

One process measures both sides, alternating them run by run (every run on a fresh copy of the
first cloud, created outside the timed region); after --warm unrecorded runs of each side the
medians of --runs runs are written to profiles/built_map_timing.json with a bit-for-bit comparison
of the two sides' results.

    python tools/built_map_timing.py [--out profiles/built_map_timing.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicp_mapping_amd import synthetic as sy  # noqa: E402

FREQ, MAX_CORR, CROP, RES, SEED = 5, 1.0, 15.0, 0.2, 1


def _cloud(a):
    """Cloud i along x, sampled out to 15 m (inside its crop) and cut to n_points. i = -1: the first
    cloud, in the map frame at the start; i >= 0: reading i in the drifted odometry frame with its
    prior pose (0.3 m and 1 degree of yaw per reading, as tools/localization_timing.py)."""
    i, n_points = a
    scene = sy.make_scene(SEED)
    o_w = np.array([(i + 1) * 0.3, 0.0, 0.7])
    rng = np.random.default_rng(SEED * 7919 + 5000 + i + 1)
    w = sy._subsample_raster(sy.sample_scene(scene, rng, o_w, half=15.0), n_points, rng)
    if i < 0:
        return w.astype(np.float32), np.eye(4)
    Ti = np.linalg.inv(sy.T_GT)
    read = (w @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return read, Ti @ sy.make_T(yaw_deg=1.0 * i, pitch_deg=0.0, roll_deg=0.0, t=o_w)


def workload(n_first, n_readings, n_points):
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        cl = list(ex.map(_cloud, [(-1, n_first)] + [(i, n_points) for i in range(n_readings)]))
    return cl[0][0], [c[0] for c in cl[1:]], [c[1] for c in cl[1:]]


def mul4(A, B):
    """Eigen Matrix4f product in float, each coefficient summed over k in order."""
    C = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            s = np.float32(A[r, 0] * B[0, c])
            for k in range(1, 4):
                s = np.float32(s + np.float32(A[r, k] * B[k, c]))
            C[r, c] = s
    return C


def moved_origin(T, o):
    """Translation of fromMatrix4fToIsometry3d(T) * prior pose (common.cpp:4-23): the float
    quaternion of T's rotation (trace branch: a small rotation), back to a rotation in double."""
    f = np.float32
    m = np.asarray(T, np.float32)[:3, :3]
    t = f(f(m[0, 0] + m[1, 1]) + m[2, 2])
    assert t > 0
    t = f(np.sqrt(f(t + f(1))))
    w = f(f(0.5) * t)
    t = f(f(0.5) / t)
    x, y, z = f(f(m[2, 1] - m[1, 2]) * t), f(f(m[0, 2] - m[2, 0]) * t), f(f(m[1, 0] - m[0, 1]) * t)
    x, y, z, w = float(x), float(y), float(z), float(w)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
         [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
    return np.array([((R[r][0] * o[0] + R[r][1] * o[1]) + R[r][2] * o[2]) + float(np.float32(T[r][3])) for r in range(3)])


def composition(ctx, L, pm, reads, poses, debug, ph):
    n, p, acc = len(reads), 0, 0
    Ts, flags = [], []
    mc = np.float32(MAX_CORR)
    initT = np.eye(4, dtype=np.float32)
    while p < n:
        w = 1 if debug else min(n - p, 4096, FREQ - acc)
        t0 = time.perf_counter()
        batch = [ctx.transform(initT, reads[p])] if debug else reads[p:p + w]
        t1 = time.perf_counter()
        pairs = []
        for i in range(w):
            P = np.asarray(poses[p + i], np.float64)
            o = P[:3, 3]
            pairs.append(dict(ref=pm.crop(-CROP, CROP, P), read=batch[i],
                              ref_origin=np.asarray(P, np.float32)[:3, 3].astype(np.float64),
                              read_origin=moved_origin(initT, o) if debug else o))
        t2 = time.perf_counter()
        T, st, rc = ctx.align_batch(pairs, resolution=RES, flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP)
        t3 = time.perf_counter()
        ph["move_ms"] += 1e3 * (t1 - t0)
        ph["crop_ms"] += 1e3 * (t2 - t1)
        ph["align_ms"] += 1e3 * (t3 - t2)
        ph["windows"] += 1
        for i in range(w):
            Ts.append(T[i])
            f = [0, 0]
            flags.append(f)
            if any(abs(T[i][k, 3]) > mc for k in range(3)):
                continue
            f[0] = 1
            acc += 1
            if acc == FREQ:
                t0 = time.perf_counter()
                pm.merge(batch[i], T[i])
                ph["merge_ms"] += 1e3 * (time.perf_counter() - t0)
                ph["appends"] += 1
                f[1] = 1
                acc = 0
            initT = mul4(T[i], initT)
        p += w
    return np.stack(Ts), flags, None


def digest(T, flags, final):
    h = hashlib.sha256()
    for a in (np.ascontiguousarray(T, np.float32), np.asarray(flags, np.int32), np.ascontiguousarray(final, np.float32)):
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def one_run(side, ctx, L, first, reads, poses, debug):
    from aicp_mapping_amd.built_map import BuiltMap

    bm = BuiltMap(ctx, first)
    ph = dict(windows=0, appends=0)
    if side == "stream":
        prm = L.default_built_map_params(reference_update_frequency=FREQ, max_correction_magnitude=MAX_CORR,
                                         crop_min=-CROP, crop_max=CROP, resolution=RES, debug=debug)
        t0 = time.perf_counter()
        T, res, done, rc = bm.sequence_run(reads, poses, params=prm)
        dt = 1e3 * (time.perf_counter() - t0)
        assert rc == 0 and done == len(reads)
        ph.update(ctx.last_built_map_timing())
        flags = [[r["accepted"], r["is_reference"]] for r in res]
        ovl = [r["icp"]["overlap_percent"] for r in res]
    else:
        ph.update(move_ms=0.0, crop_ms=0.0, align_ms=0.0, merge_ms=0.0)
        t0 = time.perf_counter()
        T, flags, ovl = composition(ctx, L, bm, reads, poses, debug, ph)
        dt = 1e3 * (time.perf_counter() - t0)
    final = bm.getCloud()
    bm.free()
    return dt, ph, T, flags, final, ovl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "built_map_timing.json"))
    ap.add_argument("--first", type=int, default=120000)
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    first, reads, poses = workload(a.first, a.readings, a.points)
    import aicp_mapping_amd._lib as L

    ctx = L.Context(0)
    out = dict(workload=dict(first_cloud_points=int(len(first)), readings=len(reads), points=int(len(reads[0])), crop=CROP,
                             reference_update_frequency=FREQ, max_correction_magnitude=MAX_CORR, resolution=RES),
               library=L.build_info(), warm=a.warm, runs=a.runs, order="stream, composition alternating, run by run",
               modes={})
    for mode in ("robot", "debug"):
        debug = mode == "debug"
        ts = dict(stream=[], composition=[])
        phs = dict(stream=[], composition=[])
        dg, last = {}, {}
        for k in range(a.warm + a.runs):
            for side in ("stream", "composition"):
                dt, ph, T, flags, final, ovl = one_run(side, ctx, L, first, reads, poses, debug)
                d = digest(T, flags, final)
                assert dg.get(side) in (None, d), f"two {side} runs differ"
                dg[side] = d
                last[side] = (T, flags, final, ovl)
                if k >= a.warm:
                    ts[side].append(dt)
                    phs[side].append(ph)
        T, flags, final, ovl = last["stream"]
        Tc, flagsc, finalc, _ = last["composition"]
        m = dict(same_results=dg["stream"] == dg["composition"],
                 same_T=bool(np.array_equal(T, Tc)), same_decisions=flags == flagsc,
                 same_final_map=bool(np.array_equal(final, finalc)),
                 max_abs_T_difference=float(np.abs(np.asarray(T) - np.asarray(Tc)).max()),
                 accepted=int(sum(f[0] for f in flags)), references=int(sum(f[1] for f in flags)),
                 final_map_points=int(len(final)), overlap_percent_min_max=[float(min(ovl)), float(max(ovl))], sides={})
        for side in ("stream", "composition"):
            m["sides"][side] = dict(wall_ms=dict(median=statistics.median(ts[side]), min=min(ts[side]), max=max(ts[side]),
                                                 all=[round(t, 3) for t in ts[side]]),
                                    phases={k: statistics.median(p[k] for p in phs[side]) for k in phs[side][0]},
                                    digest=dg[side])
        m["composition_over_stream"] = m["sides"]["composition"]["wall_ms"]["median"] / m["sides"]["stream"]["wall_ms"]["median"]
        out["modes"][mode] = m
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
