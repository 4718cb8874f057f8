"""Time App's localization stream (PriorMap.sequence_run, aicp_hip_map_sequence_run) on a C4-size
workload against the hand composition of the entry points that served it before: one
register_batch per window, then merge (the reading uploaded a second time) and prefilter, with
App's counters kept on the host. Workload: a 1 M-point map, 64 readings of 120 k points, crop
-15..15, a merge every 5 accepted readings, a re-filter every 30; robot and debug working mode.

A process measures one side with the library it loaded, so the composition can run on an older
library (AICP_HIP_LIB) that has no stream entry point:

    python tools/localization_timing.py --part stream --out a.json
    AICP_HIP_LIB=old.so python tools/localization_timing.py --part composition --out b.json
    python tools/localization_timing.py --combine a.json b.json [more parts...]

Each part: medians of warmed runs (every run on a fresh copy of the map, created outside the timed
region). --combine takes the median over the parts of a side (alternate the sides when you run
them) and writes profiles/localization_timing.json.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicp_mapping_amd import synthetic as sy  # noqa: E402

FREQ, REFILTER, MAX_CORR, CROP = 5, 30, 1.0, 15.0


def _map(seed, n_map):
    scene = sy.make_scene(seed)
    rng = np.random.default_rng(seed * 7919 + 77)
    mp = sy.sample_scene(scene, rng, np.array([0.0, 0.0, 0.7]), half=40.0)
    return mp[rng.choice(len(mp), size=min(n_map, len(mp)), replace=False)].astype(np.float32)


def _reading(a):
    """Reading i of a stream along x in the drifted odometry frame and its prior pose (as the C4
    readings of tests/test_configs.py, 0.3 m and 1 degree of yaw per reading), sampled out to 15 m
    so that the reading lies inside its crop: with readings out to 30 m three quarters of a reading
    fall outside the crop, more than the fixed 50 % trim removes, and most registrations slide
    along the scene and are dropped (measured: 17 of 64 accepted)."""
    seed, i, n_points = a
    scene = sy.make_scene(seed)
    Ti = np.linalg.inv(sy.T_GT)
    o_w = np.array([(i + 1) * 0.3, 0.0, 0.7])
    rng = np.random.default_rng(seed * 7919 + 5000 + i)
    w = sy._subsample_raster(sy.sample_scene(scene, rng, o_w, half=15.0), n_points, rng)
    read = (w @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return read, Ti @ sy.make_T(yaw_deg=1.0 * i, pitch_deg=0.0, roll_deg=0.0, t=o_w)


def workload(n_map, n_readings, n_points, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["map"], [z[f"r{i}"] for i in range(n_readings)], [z[f"p{i}"] for i in range(n_readings)]
    mp = _map(1, n_map)
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        rd = list(ex.map(_reading, [(1, i, n_points) for i in range(n_readings)]))
    reads, poses = [r[0] for r in rd], [r[1] for r in rd]
    if cache:
        np.savez(cache, map=mp, **{f"r{i}": r for i, r in enumerate(reads)}, **{f"p{i}": p for i, p in enumerate(poses)})
    return mp, reads, poses


def window(n_clouds, debug, remaining):
    """aicp_hip_localization_window's rule, restated (an older library does not export it)."""
    if debug:
        return 1
    k = min(remaining, 4096)
    for period in (FREQ, REFILTER):
        r = n_clouds % period
        k = min(k, 1 if r == 0 else period - r + 1)
    return k


def mul4(A, B):
    C = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            s = np.float32(A[r, 0] * B[0, c])
            for k in range(1, 4):
                s = np.float32(s + np.float32(A[r, k] * B[k, c]))
            C[r, c] = s
    return C


def composition(ctx, pm, reads, poses, debug, ph):
    n, p, n_clouds = len(reads), 0, 0
    Ts, flags = [], []
    mc = np.float32(MAX_CORR)
    initT = np.eye(4, dtype=np.float32)
    while p < n:
        w = window(n_clouds, debug, n - p)
        t0 = time.perf_counter()
        batch = [ctx.transform(initT, reads[p])] if debug else reads[p:p + w]
        t1 = time.perf_counter()
        T, st, rc = pm.register_batch(batch, poses[p:p + w], -CROP, CROP)
        t2 = time.perf_counter()
        ph["move_ms"] += 1e3 * (t1 - t0)
        ph["register_ms"] += 1e3 * (t2 - t1)
        ph["windows"] += 1
        for i in range(w):
            Ts.append(T[i])
            f = [0, 0, 0]
            flags.append(f)
            if n_clouds != 0 and any(abs(T[i][k, 3]) > mc for k in range(3)):
                continue
            n_clouds += 1
            f[0] = 1
            initT = mul4(T[i], initT)
            if (n_clouds - 1) % FREQ == 0:
                t0 = time.perf_counter()
                pm.merge(batch[i], T[i])
                ph["merge_ms"] += 1e3 * (time.perf_counter() - t0)
                ph["merges"] += 1
                f[1] = 1
            if (n_clouds - 1) % REFILTER == 0:
                t0 = time.perf_counter()
                pm.prefilter()
                ph["refilter_ms"] += 1e3 * (time.perf_counter() - t0)
                ph["refilters"] += 1
                f[2] = 1
        p += w
    return np.stack(Ts), flags


def digest(T, flags, final):
    h = hashlib.sha256()
    for a in (np.ascontiguousarray(T, np.float32), np.asarray(flags, np.int32), np.ascontiguousarray(final, np.float32)):
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def measure(part, mp, reads, poses, warm, runs):
    import aicp_mapping_amd._lib as L
    from aicp_mapping_amd.prior_map import PriorMap

    ctx = L.Context(0)
    rec = dict(part=part, library=L.build_info(), library_path=os.path.abspath(L.LIB_PATH), modes={})
    for mode in ("robot", "debug"):
        debug = mode == "debug"
        ts, phs, dg = [], [], None
        for k in range(warm + runs):
            pm = PriorMap(ctx, mp)
            ph = dict(windows=0, merges=0, refilters=0)
            if part == "stream":
                prm = L.default_localization_params(reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                                                    max_correction_magnitude=MAX_CORR, crop_min=-CROP, crop_max=CROP,
                                                    debug=debug)
                t0 = time.perf_counter()
                T, res, done, rc = pm.sequence_run(reads, poses, params=prm)
                dt = 1e3 * (time.perf_counter() - t0)
                assert rc == 0 and done == len(reads)
                ph.update(ctx.last_localization_timing())
                flags = [[r["accepted"], r["merged"], r["refiltered"]] for r in res]
            else:
                ph.update(move_ms=0.0, register_ms=0.0, merge_ms=0.0, refilter_ms=0.0)
                t0 = time.perf_counter()
                T, flags = composition(ctx, pm, reads, poses, debug, ph)
                dt = 1e3 * (time.perf_counter() - t0)
            final = pm.getCloud()
            pm.free()
            d = digest(T, flags, final)
            assert dg in (None, d), "two runs of one side differ"
            dg = d
            if k >= warm:
                ts.append(dt)
                phs.append(ph)
        rec["modes"][mode] = dict(wall_ms=dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts)),
                                  phases={k: statistics.median(p[k] for p in phs) for k in phs[0]},
                                  accepted=int(sum(f[0] for f in flags)), accepted_flags=[int(f[0]) for f in flags],
                                  translations=[[round(float(v), 3) for v in t[:3, 3]] for t in T],
                                  final_map_points=int(len(final)), digest=dg)
    ctx.close()
    return rec


def combine(paths):
    parts = [json.load(open(p)) for p in paths]
    out = dict(workload=parts[0]["workload"], runs_per_part=parts[0]["runs"], sides={}, same_results={})
    for side in ("stream", "composition"):
        ps = [p for p in parts if p["part"] == side]
        if not ps:
            continue
        out["sides"][side] = dict(library=ps[0]["library"], parts=len(ps), modes={})
        for mode in ("robot", "debug"):
            ms = [p["modes"][mode] for p in ps]
            out["sides"][side]["modes"][mode] = dict(
                median_ms=statistics.median(m["wall_ms"]["median_ms"] for m in ms),
                part_medians_ms=[m["wall_ms"]["median_ms"] for m in ms],
                min_ms=min(m["wall_ms"]["min_ms"] for m in ms), max_ms=max(m["wall_ms"]["max_ms"] for m in ms),
                phases=ms[-1]["phases"], accepted=ms[-1]["accepted"], final_map_points=ms[-1]["final_map_points"],
                digest=ms[-1]["digest"])
    if len(out["sides"]) == 2:
        for mode in ("robot", "debug"):
            a, b = (out["sides"][s]["modes"][mode] for s in ("stream", "composition"))
            out["same_results"][mode] = a["digest"] == b["digest"]
            out.setdefault("speedup", {})[mode] = b["median_ms"] / a["median_ms"]
    with open(os.path.join(ROOT, "profiles", "localization_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("stream", "composition"))
    ap.add_argument("--combine", nargs="+")
    ap.add_argument("--out")
    ap.add_argument("--map", type=int, default=1000000)
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "localization_timing_workload.npz"))
    ap.add_argument("--gen-only", action="store_true")
    a = ap.parse_args()
    if a.combine:
        return combine(a.combine)
    mp, reads, poses = workload(a.map, a.readings, a.points, a.cache)
    if a.gen_only:
        print(len(mp), [len(r) for r in reads[:3]])
        return
    rec = measure(a.part, mp, reads, poses, a.warm, a.runs)
    rec.update(workload=dict(map_points=int(len(mp)), readings=len(reads), points=int(len(reads[0])), crop=CROP,
                             reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                             max_correction_magnitude=MAX_CORR), runs=a.runs, warm=a.warm)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
