"""Time the two map localization streams on RAW readings (PriorMap / BuiltMap .sequence_run(raw=True):
aicp_hip_map_sequence_run_raw, aicp_hip_built_map_sequence_run_raw) against the hand composition
through the entry points that served raw readings before: aicp_hip_prefilter per reading (the kept
points come back to the host), then the pre-filtered stream (which uploads them again). The
composition uses none of the new entry points, so its time is the previous commit's on this build.

Workloads, as tools/localization_timing.py and tools/built_map_timing.py: a 1 M-point map (built
map: a 120 k-point first cloud), 64 readings, crop -15..15, a merge / reference every 5 accepted
readings, a re-filter every 30 (prior map), octree 0.2 m (built map). The readings are raw: the
scene sampled at 0.05 m out to 10.7 m, which the pre-filter brings to about 120 k points.

Per stream and working mode one process measures the sides, alternating them run by run (every
run on a fresh copy of the map, created outside the timed region); after --warm unrecorded rounds
the medians of --runs rounds go to profiles/raw_localization_timing.json:

  robot mode   raw stream | composition (per-reading prefilter + pre-filtered stream); the results
               are compared bit for bit
  debug mode   raw stream (App's order: move, then filter). No composition exists for it; beside it
               the pre-filtered debug stream on readings filtered beforehand (the swapped order, other
               points), with and without the time of that filtering

Also the ingest of one reading of --ingest-points rows (2.57 M: the C2 raw size), both forms through
aicp_hip_test_ingest without its download: 16-byte rows uploaded verbatim and unpacked by
k_stream_ingest, against 32-byte rows packed on the host first (pack, upload, the same kernel at
stride 16); 12-byte rows verbatim beside them.

    python tools/raw_localization_timing.py [--out profiles/raw_localization_timing.json]
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

FREQ, REFILTER, MAX_CORR, CROP, RES, SEED = 5, 30, 1.0, 15.0, 0.2, 1
HALF, SPACING = 10.7, 0.05


def _map(n_map):
    scene = sy.make_scene(SEED)
    rng = np.random.default_rng(SEED * 7919 + 77)
    mp = sy.sample_scene(scene, rng, np.array([0.0, 0.0, 0.7]), half=40.0)
    return mp[rng.choice(len(mp), size=min(n_map, len(mp)), replace=False)].astype(np.float32)


def _first(n_first):
    scene = sy.make_scene(SEED)
    rng = np.random.default_rng(SEED * 7919 + 5000)
    return sy._subsample_raster(sy.sample_scene(scene, rng, np.array([0.0, 0.0, 0.7]), half=15.0), n_first,
                                rng).astype(np.float32)


def _raw_reading(i):
    """Raw reading i of a stream along x in the drifted odometry frame and its prior pose (0.3 m and
    1 degree of yaw per reading, as tools/localization_timing.py), every sampled point kept."""
    scene = sy.make_scene(SEED)
    Ti = np.linalg.inv(sy.T_GT)
    o_w = np.array([(i + 1) * 0.3, 0.0, 0.7])
    rng = np.random.default_rng(SEED * 7919 + 5000 + i + 1)
    w = sy.sample_scene(scene, rng, o_w, half=HALF, spacing=SPACING)
    read = (w @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return read, Ti @ sy.make_T(yaw_deg=1.0 * i, pitch_deg=0.0, roll_deg=0.0, t=o_w)


def workload(n_readings):
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        rd = list(ex.map(_raw_reading, range(n_readings)))
    return [r[0] for r in rd], [r[1] for r in rd]


def digest(T, res, final, append):
    h = hashlib.sha256()
    flags = [[r["status"], r["accepted"], r[append], r["crop_points"], r["icp"]["iterations"]] for r in res]
    for a in (np.ascontiguousarray(T, np.float32), np.asarray(flags, np.int64), np.ascontiguousarray(final, np.float32)):
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def measure_stream(L, ctx, stream, mp, raws, poses, warm, runs):
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.prior_map import PriorMap

    cls, append = (PriorMap, "merged") if stream == "prior" else (BuiltMap, "is_reference")

    def prm(debug):
        if stream == "prior":
            return L.default_localization_params(reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                                                 max_correction_magnitude=MAX_CORR, crop_min=-CROP, crop_max=CROP,
                                                 debug=debug)
        return L.default_built_map_params(reference_update_frequency=FREQ, max_correction_magnitude=MAX_CORR,
                                          crop_min=-CROP, crop_max=CROP, resolution=RES, debug=debug)

    def raw_side(debug):
        m = cls(ctx, mp)
        t0 = time.perf_counter()
        T, res, done, rc, kept = m.sequence_run(raws, poses, params=prm(debug), raw=True, raise_on_error=False)
        dt = 1e3 * (time.perf_counter() - t0)
        final = m.getCloud()
        m.free()
        return dict(ms=dt, rc=rc, done=done, digest=digest(T, res, final, append),
                    accepted=int(sum(r["accepted"] for r in res)), appended=int(sum(r[append] for r in res)),
                    kept=[int(k) for k in kept], final_map_points=len(final))

    def composed_side(debug):
        m = cls(ctx, mp)
        t0 = time.perf_counter()
        kept = [ctx.prefilter(r) for r in raws]
        t1 = time.perf_counter()
        T, res, done, rc = m.sequence_run(kept, poses, params=prm(debug), raise_on_error=False)
        t2 = time.perf_counter()
        final = m.getCloud()
        m.free()
        return dict(ms=1e3 * (t2 - t0), stream_ms=1e3 * (t2 - t1), rc=rc, done=done,
                    digest=digest(T, res, final, append),
                    accepted=int(sum(r["accepted"] for r in res)), appended=int(sum(r[append] for r in res)),
                    kept=[len(k) for k in kept], final_map_points=len(final))

    sides = [("robot", "raw_stream", raw_side, False), ("robot", "composition", composed_side, False),
             ("debug", "raw_stream", raw_side, True), ("debug", "prefiltered_stream", composed_side, True)]
    recs = {(mode, name): [] for mode, name, _, _ in sides}
    for k in range(warm + runs):
        order = sides if k % 2 == 0 else sides[::-1]
        for mode, name, fn, debug in order:
            r = fn(debug)
            if recs[(mode, name)]:
                assert recs[(mode, name)][-1]["digest"] == r["digest"], "two runs of one side differ"
            if k >= warm or not recs[(mode, name)]:
                recs[(mode, name)].append(r)
    out = {}
    for (mode, name), rs in recs.items():
        rs = rs[-runs:]
        last = rs[-1]
        e = dict(wall_ms=spread([r["ms"] for r in rs]), rc=last["rc"], readings_done=last["done"],
                 accepted=last["accepted"], appended=last["appended"],
                 kept_median=int(statistics.median(last["kept"])), kept_min=min(last["kept"]), kept_max=max(last["kept"]),
                 final_map_points=last["final_map_points"], digest=last["digest"])
        if "stream_ms" in last:
            e["stream_only_ms"] = spread([r["stream_ms"] for r in rs])
        out.setdefault(mode, {})[name] = e
    rb = out["robot"]
    rb["same_results"] = rb["raw_stream"]["digest"] == rb["composition"]["digest"]
    rb["same_kept"] = recs[("robot", "raw_stream")][-1]["kept"] == recs[("robot", "composition")][-1]["kept"]
    rb["composition_over_raw_stream"] = rb["composition"]["wall_ms"]["median_ms"] / rb["raw_stream"]["wall_ms"]["median_ms"]
    return out


def measure_ingest(ctx, n_points, warm, runs):
    g = np.random.default_rng(3)
    p3 = (g.standard_normal((n_points, 3)) * 10.0).astype(np.float32)
    forms = dict(rows12_verbatim=p3, rows16_verbatim=np.concatenate([p3, np.ones((n_points, 1), np.float32)], 1),
                 rows32_host_packed=np.concatenate([p3, np.zeros((n_points, 5), np.float32)], 1))
    ts = {k: [] for k in forms}
    for k in range(warm + runs):
        names = list(forms) if k % 2 == 0 else list(forms)[::-1]
        for name in names:
            t0 = time.perf_counter()
            ctx.test_ingest(forms[name], download=False)
            if k >= warm:
                ts[name].append(1e3 * (time.perf_counter() - t0))
    out = dict(points=n_points, forms={k: spread(v) for k, v in ts.items()})
    out["verbatim_16_not_slower_than_host_pack"] = (out["forms"]["rows16_verbatim"]["median_ms"] <=
                                                    out["forms"]["rows32_host_packed"]["median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_localization_timing.json"))
    ap.add_argument("--map", type=int, default=1000000)
    ap.add_argument("--first", type=int, default=120000)
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--ingest-points", type=int, default=2570000)
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L

    raws, poses = workload(a.readings)
    ctx = L.Context(0)
    out = dict(library=L.build_info(), runs=a.runs, warm=a.warm,
               workload=dict(readings=len(raws), raw_points_median=int(statistics.median(len(r) for r in raws)),
                             half=HALF, spacing=SPACING, crop=CROP, reference_update_frequency=FREQ,
                             map_refilter_every=REFILTER, max_correction_magnitude=MAX_CORR, resolution=RES),
               streams={})
    mp = _map(a.map)
    out["workload"]["prior_map_points"] = int(len(mp))
    out["streams"]["prior_map"] = measure_stream(L, ctx, "prior", mp, raws, poses, a.warm, a.runs)
    print(json.dumps(out["streams"]["prior_map"]), flush=True)
    first = ctx.prefilter(_first(a.first))  # App's first cloud, pre-filtered
    out["workload"]["built_map_first_points"] = int(len(first))
    out["streams"]["built_map"] = measure_stream(L, ctx, "built", first, raws, poses, a.warm, a.runs)
    print(json.dumps(out["streams"]["built_map"]), flush=True)
    out["ingest"] = measure_ingest(ctx, a.ingest_points, a.warm, a.runs)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
