"""Time the live map sessions (MapSession: aicp_hip_map_session_*) per reading, on the workload of
tools/raw_localization_timing.py: a resident 1 M-point map (built map: a 120 k-point first cloud),
64 raw readings of about 277 k points, crop -15..15, a merge / reference every 5 accepted readings,
a re-filter every 30 (prior map), octree 0.2 m (built map).

Both policies and both working modes in one process; inside every round the variants alternate
(every run on a fresh copy of the map, created outside the timed region). After --warm unrecorded
rounds the medians of --runs rounds, with (min, max), go to profiles/map_session_timing.json, all as
milliseconds per reading:

  session      MapSession.process, reading by reading
  stream       the offline *_run_raw stream over the whole recording, divided by the readings. In
               debug mode its windows are one reading long: the same device work reading by reading,
               the baseline. In robot mode it batches the readings between two map changes, which a
               live node cannot do (it does not have the next reading yet): a lower bound, not a rival
  composition  prior map, robot mode only: what a node had to write before the session existed:
               ctx.prefilter (kept points down), PriorMap.register_batch of one reading (up again),
               App's rules on the host, PriorMap.merge (up a third time) / PriorMap.prefilter

The tool asserts the sameness it reports: the session against the debug-mode stream bit for bit
(corrections, records, kept counts, final map), against the composition bit for bit (corrections,
decisions, final map), and against the robot-mode stream in every decision and the final map's size.

    python tools/map_session_timing.py [--out profiles/map_session_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import raw_localization_timing as rl  # noqa: E402  (the workload, unchanged)

FREQ, REFILTER, MAX_CORR, CROP, RES = rl.FREQ, rl.REFILTER, rl.MAX_CORR, rl.CROP, rl.RES


def measure(L, ctx, policy, mp, raws, poses, warm, runs):
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.prior_map import PriorMap

    cls, append = (PriorMap, "merged") if policy == "prior" else (BuiltMap, "is_reference")
    n = len(raws)

    def prm(debug):
        if policy == "prior":
            return L.default_localization_params(reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                                                 max_correction_magnitude=MAX_CORR, crop_min=-CROP, crop_max=CROP,
                                                 debug=debug)
        return L.default_built_map_params(reference_update_frequency=FREQ, max_correction_magnitude=MAX_CORR,
                                          crop_min=-CROP, crop_max=CROP, resolution=RES, debug=debug)

    def record(ms, T, res, kept, final, rc):
        return dict(ms=ms / n, rc=rc, done=len(res), digest=rl.digest(T, res, final, append),
                    decisions=[[r["status"], r["accepted"], r[append], r.get("refiltered", 0)] for r in res],
                    T=np.ascontiguousarray(T, np.float32), final=final, kept=[int(k) for k in kept])

    def session_side(debug):
        m = cls(ctx, mp)
        s = MapSession(ctx, m, params=prm(debug), prefilter=True)
        s.start()
        T, res, kept, rc = [], [], [], 0
        t0 = time.perf_counter()
        for r, P in zip(raws, poses):
            t, d, k = s.process(r, P, raise_on_error=False)
            T.append(t)
            res.append(d)
            kept.append(k)
            if d["rc"]:
                rc = d["rc"]
                break
        dt = 1e3 * (time.perf_counter() - t0)
        for d in res:
            d.pop("rc")
        final = m.getCloud()
        s.close()
        m.free()
        return record(dt, T, res, kept, final, rc)

    def stream_side(debug):
        m = cls(ctx, mp)
        t0 = time.perf_counter()
        T, res, done, rc, kept = m.sequence_run(raws, poses, params=prm(debug), raw=True, raise_on_error=False)
        dt = 1e3 * (time.perf_counter() - t0)
        final = m.getCloud()
        m.free()
        return record(dt, T[:done], res, kept, final, rc)

    def composed_side(debug):
        """App's prior-map rules on the host (app.cpp:366-373, 469-493), robot mode."""
        m = cls(ctx, mp)
        T, res, kept, n_clouds = [], [], [], 0
        t0 = time.perf_counter()
        for r, P in zip(raws, poses):
            k = ctx.prefilter(r)
            t, st, rc = m.register_batch([k], [P], mn=-CROP, mx=CROP)
            t = t[0]
            d = dict(status=rc, accepted=0, merged=0, refiltered=0, crop_points=0, icp=st[0])
            T.append(t)
            res.append(d)
            kept.append(len(k))
            if n_clouds != 0 and any(abs(t[i, 3]) > np.float32(MAX_CORR) for i in range(3)):
                continue
            n_clouds += 1
            d["accepted"] = 1
            if (n_clouds - 1) % FREQ == 0:
                m.merge(k, t)
                d["merged"] = 1
            if (n_clouds - 1) % REFILTER == 0:
                m.prefilter()
                d["refiltered"] = 1
        dt = 1e3 * (time.perf_counter() - t0)
        final = m.getCloud()
        m.free()
        out = record(dt, T, res, kept, final, 0)
        return out

    sides = [("robot", "session", session_side, False), ("robot", "stream", stream_side, False),
             ("debug", "session", session_side, True), ("debug", "stream", stream_side, True)]
    if policy == "prior":
        sides.insert(2, ("robot", "composition", composed_side, False))
    recs = {(mode, name): [] for mode, name, _, _ in sides}
    for k in range(warm + runs):
        order = sides if k % 2 == 0 else sides[::-1]
        for mode, name, fn, debug in order:
            r = fn(debug)
            if recs[(mode, name)]:
                assert recs[(mode, name)][-1]["digest"] == r["digest"], "two runs of one variant differ"
            if k >= warm or not recs[(mode, name)]:
                for old in recs[(mode, name)]:  # (only the last run's arrays are compared)
                    old["T"] = old["final"] = None
                recs[(mode, name)].append(r)
    out = {}
    for (mode, name), rs in recs.items():
        rs, last = rs[-runs:], rs[-1]
        out.setdefault(mode, {})[name] = dict(
            per_reading_ms=rl.spread([r["ms"] for r in rs]), rc=last["rc"], readings_done=last["done"],
            accepted=int(sum(d[1] for d in last["decisions"])), appended=int(sum(d[2] for d in last["decisions"])),
            refiltered=int(sum(d[3] for d in last["decisions"])), kept_median=int(statistics.median(last["kept"])),
            final_map_points=int(len(last["final"])), digest=last["digest"])
    # the sameness this tool claims
    s, b = recs[("debug", "session")][-1], recs[("debug", "stream")][-1]
    assert s["digest"] == b["digest"] and s["kept"] == b["kept"] and s["decisions"] == b["decisions"], \
        "debug mode: the session differs from the stream"
    out["debug"]["session_equals_stream_bit_for_bit"] = True
    s, b = recs[("robot", "session")][-1], recs[("robot", "stream")][-1]
    assert (s["decisions"] == b["decisions"] and s["kept"] == b["kept"] and len(s["final"]) == len(b["final"])), \
        "robot mode: the session decides differently from the stream"
    out["robot"]["session_decides_as_stream"] = True
    out["robot"]["session_equals_stream_bit_for_bit"] = s["digest"] == b["digest"]  # (reported, not required)
    if policy == "prior":
        c = recs[("robot", "composition")][-1]
        assert (np.array_equal(s["T"].view(np.uint32), c["T"].view(np.uint32)) and s["decisions"] == c["decisions"] and
                s["kept"] == c["kept"] and s["final"].tobytes() == c["final"].tobytes()), \
            "robot mode: the session differs from the hand composition"
        out["robot"]["session_equals_composition_bit_for_bit"] = True
        out["robot"]["composition_over_session"] = (out["robot"]["composition"]["per_reading_ms"]["median_ms"] /
                                                    out["robot"]["session"]["per_reading_ms"]["median_ms"])
    for mode in ("robot", "debug"):
        out[mode]["session_over_stream"] = (out[mode]["session"]["per_reading_ms"]["median_ms"] /
                                            out[mode]["stream"]["per_reading_ms"]["median_ms"])
    base = out["debug"]["stream"]["per_reading_ms"]
    out["debug"]["session_median_within_baseline_range_or_below"] = bool(
        out["debug"]["session"]["per_reading_ms"]["median_ms"] <= base["max_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_session_timing.json"))
    ap.add_argument("--map", type=int, default=1000000)
    ap.add_argument("--first", type=int, default=120000)
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L

    raws, poses = rl.workload(a.readings)
    ctx = L.Context(0)
    out = dict(library=L.build_info(), runs=a.runs, warm=a.warm, unit="ms per reading",
               workload=dict(readings=len(raws), raw_points_median=int(statistics.median(len(r) for r in raws)),
                             half=rl.HALF, spacing=rl.SPACING, crop=CROP, reference_update_frequency=FREQ,
                             map_refilter_every=REFILTER, max_correction_magnitude=MAX_CORR, resolution=RES),
               notes=dict(debug_stream="one reading per window: the baseline",
                          robot_stream="batches the readings between two map changes: a lower bound a live node "
                                       "cannot reach"),
               policies={})
    mp = rl._map(a.map)
    out["workload"]["prior_map_points"] = int(len(mp))
    out["policies"]["prior_map"] = measure(L, ctx, "prior", mp, raws, poses, a.warm, a.runs)
    print(json.dumps(out["policies"]["prior_map"]), flush=True)
    first = ctx.prefilter(rl._first(a.first))  # App's first cloud, pre-filtered
    out["workload"]["built_map_first_points"] = int(len(first))
    out["policies"]["built_map"] = measure(L, ctx, "built", first, raws, poses, a.warm, a.runs)
    print(json.dumps(out["policies"]["built_map"]), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
