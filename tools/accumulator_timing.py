"""Time the assembly of one C2-size raw reading from lidar sweeps: the sweep accumulator
(SweepAccumulator, aicp_hip_accum_*) against the composition of the entry points that a caller had
before it. Workload: 80 sweeps of 32 k points (2.56 M raw points), each in its own sensor frame
under its own pose, cropped to +-30 m, moved and concatenated, then pre-filtered.

  accumulator   80 x push, then prefilter() on the device-resident cloud. Reported: the host time
                inside the 80 push calls, first push -> stream idle, first push -> kept points on
                the host.
  composition   per sweep Context.crop_box and Context.transform (aicp_hip_crop_box,
                aicp_hip_transform: an upload, the kernels and a download each), a host
                concatenate, then Context.prefilter of the whole (aicp_hip_prefilter).

    python tools/accumulator_timing.py                      # both sides, alternating
    python tools/accumulator_timing.py --side accumulator   # one side (for a kernel trace)
    python tools/accumulator_timing.py --stats-csv kernel_stats.csv   # add a trace's kernel times

Medians of warmed runs; both sides must return the same points, bit for bit. Writes
profiles/accumulator_timing.json (--out).
"""
import argparse
import csv
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicp_mapping_amd import synthetic as sy  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "accumulator_timing.json")


def workload(n_sweeps, n_points, seed=1):
    """The scene out to 34 m around the sensor (so the +-30 m crop drops about a fifth), dealt at
    random into n_sweeps sweeps of n_points; sweep i is seen from a pose 2 cm and 0.1 degree of yaw
    further along than sweep i - 1 and is given in that sensor frame."""
    rng = np.random.default_rng(seed * 7919 + 4242)
    w = sy.sample_scene(sy.make_scene(seed), rng, (0.0, 0.0, 0.7), half=34.0, spacing=0.04)
    total = n_sweeps * n_points
    assert len(w) >= total, (len(w), total)
    w = w[rng.choice(len(w), size=total, replace=False)]
    sweeps, poses = [], []
    for i in range(n_sweeps):
        P = sy.make_T(yaw_deg=0.1 * i, pitch_deg=0.3, roll_deg=-0.2, t=(0.02 * i, 0.0, 0.7))
        sweeps.append(sy.transform(np.linalg.inv(P), w[i * n_points:(i + 1) * n_points]))
        poses.append(P)
    return sweeps, poses


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()[:16]


def run_accumulator(acc, sweeps, poses):
    """(kept points, times in ms) of one reading: pushes and wait, then pushes and pre-filter."""
    pc = time.perf_counter
    acc.clear()
    t0 = pc()
    host = 0.0
    for s, P in zip(sweeps, poses):
        a = pc()
        acc.push(s, P)
        host += pc() - a
    n_raw = len(acc)  # waits for the stream
    t_idle = pc() - t0
    acc.clear()
    t0 = pc()
    for s, P in zip(sweeps, poses):
        acc.push(s, P)
    t1 = pc()
    kept = acc.prefilter()
    t2 = pc()
    return kept, dict(push_host_ms=1e3 * host, first_push_to_idle_ms=1e3 * t_idle, prefilter_ms=1e3 * (t2 - t1),
                      first_push_to_kept_ms=1e3 * (t2 - t0)), n_raw


def run_composition(ctx, sweeps, poses, Ts):
    pc = time.perf_counter
    eye = np.eye(4, dtype=np.float32)
    t0 = pc()
    tc = tt = 0.0
    parts = []
    for s, T in zip(sweeps, Ts):
        a = pc()
        k, _ = ctx.crop_box(s, -30.0, 30.0, eye)
        b = pc()
        parts.append(ctx.transform(T, k) if len(k) else k)
        tc += b - a
        tt += pc() - b
    a = pc()
    raw = np.concatenate(parts, axis=0)
    b = pc()
    kept = ctx.prefilter(raw)
    t2 = pc()
    return kept, dict(crop_ms=1e3 * tc, transform_ms=1e3 * tt, concatenate_ms=1e3 * (b - a), assembly_ms=1e3 * (b - t0),
                      prefilter_ms=1e3 * (t2 - b), first_sweep_to_kept_ms=1e3 * (t2 - t0)), len(raw)


def med(recs):
    return {k: statistics.median(r[k] for r in recs) for k in recs[0]}


def measure(a):
    import aicp_mapping_amd._lib as L
    from aicp_mapping_amd.accumulator import SweepAccumulator, pose_matrix

    sweeps, poses = workload(a.sweeps, a.points)
    Ts = [pose_matrix(P) for P in poses]
    ctx = L.Context(0)
    acc = SweepAccumulator(ctx, a.sweeps * a.points, batch_size=a.sweeps)
    sides = ("accumulator", "composition") if a.side == "both" else (a.side,)
    recs = {s: [] for s in sides}
    dg, n_raw, n_kept = {}, {}, {}
    for k in range(a.warm + a.runs):
        for side in sides:  # alternating
            if side == "accumulator":
                kept, t, n = run_accumulator(acc, sweeps, poses)
            else:
                kept, t, n = run_composition(ctx, sweeps, poses, Ts)
            d = digest(kept)
            assert dg.setdefault(side, d) == d, "two runs of one side differ"
            n_raw[side], n_kept[side] = int(n), int(len(kept))
            if k >= a.warm:
                recs[side].append(t)
    acc.free()
    out = dict(workload=dict(sweeps=a.sweeps, points_per_sweep=a.points, raw_points=a.sweeps * a.points,
                             cropped_points=n_raw[sides[0]], kept_points=n_kept[sides[0]]),
               runs=a.runs, warm=a.warm, library=L.build_info(),
               sides={s: dict(median_ms=med(recs[s]), cropped_points=n_raw[s], kept_points=n_kept[s], digest=dg[s])
                      for s in sides})
    if len(sides) == 2:
        out["same_results"] = dg["accumulator"] == dg["composition"] and n_raw["accumulator"] == n_raw["composition"]
        out["speedup_first_sweep_to_kept"] = (out["sides"]["composition"]["median_ms"]["first_sweep_to_kept_ms"] /
                                              out["sides"]["accumulator"]["median_ms"]["first_push_to_kept_ms"])
        out["speedup_assembly"] = (out["sides"]["composition"]["median_ms"]["assembly_ms"] /
                                   out["sides"]["accumulator"]["median_ms"]["first_push_to_idle_ms"])
    ctx.close()
    return out


def kernel_stats(path):
    """The accumulator's and the composition's per-sweep kernels from a kernel trace's statistics
    (rocprofv3 --kernel-trace --stats, taken on its own with no counters: a CSV with Name, Calls,
    AverageNs ... columns)."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("k_accum_count", "k_accum_scatter", "k_crop_count", "k_crop_scan", "k_crop_scatter", "k_transform"):
                if key + "(" in name or name.endswith(key) or ("::" + key) in name:
                    out[key] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                                    min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("both", "accumulator", "composition"), default="both")
    ap.add_argument("--sweeps", type=int, default=80)
    ap.add_argument("--points", type=int, default=32000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--stats-csv", help="add the per-sweep kernel times of a kernel trace to --out and exit")
    a = ap.parse_args()
    if a.stats_csv:
        rec = json.load(open(a.out))
        rec.setdefault("kernel_trace_us", {}).update(kernel_stats(a.stats_csv))
    else:
        rec = measure(a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
