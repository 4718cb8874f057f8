"""Time the mapping session's built map (AppSession(keep_aligned_map=True)) and the go-back against
what a caller composed before them.

Workload: the session timing tool's C2-size raw stream (64 readings of 120 k points, a reference
every 5), reading by reading, in one process, the variants alternating inside every round:

  keep_off      AppSession.process per reading, as it always was
  keep_on       the same with keep_aligned_map=True: every promotion also stored behind the map
  composition   keep_off plus what a caller did by hand for the map: reference() downloaded after
                every promotion and concatenated on the host

and, on the map each of them ends with, the go-back:

  go_back       take_aligned_map() + MapSession.start_go_back(session)
  compose_back  PriorMap(ctx, host map) (aicp_hip_map_create: the whole map up the bus) +
                MapSession.start()

Per variant: the median over rounds and the spread (min, max) of the per-reading wall and device
time, of the go-back's wall time, and the bytes of map points that crossed the bus (16 per point,
as the copies move them). The tool asserts that the three forms give the same corrections and the
same map, bit for bit. Writes profiles/mapping_timing.json (--out).

    python tools/mapping_timing.py
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
from aicp_mapping_amd import synthetic as sy  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mapping_timing.json")
pc = time.perf_counter


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.prior_map import PriorMap
    from aicp_mapping_amd.session import AppSession

    ctx = L.Context(0)
    st = sy.make_stream(n_readings=a.readings, n_points=a.points, seed=1)
    n = a.readings
    prm = L.default_sequence_params(reference_update_frequency=5, flags=L.AICP_RUN_OVERLAP)
    loc = L.default_localization_params()

    def mapping(keep, compose):
        """One mapping run: (T, host map or None, session left open, timings, bus bytes of map points)."""
        s = AppSession(ctx, params=prm, prefilter=True, keep_aligned_map=keep)
        s.start(st.first, st.first_origin)
        host = [s.reference()[0]] if compose else None
        bus = 16 * len(host[0]) if compose else 0
        wall, dev, Ts = [], [], []
        t0 = pc()
        for r, o in zip(st.readings, st.origins):
            b = pc()
            T, res, kept = s.process(r, o)
            dev.append(s.last_timing()["device_ms"])
            if compose and res["is_reference"]:
                host.append(s.reference()[0])
                bus += 16 * len(host[-1])
            wall.append(1e3 * (pc() - b))
            Ts.append(T)
        if compose:
            b = pc()
            host = np.concatenate(host, 0)
            cat = 1e3 * (pc() - b)
        total = 1e3 * (pc() - t0)
        t = dict(wall_ms_per_reading=statistics.median(wall), device_ms_per_reading=statistics.median(dev),
                 mean_wall_ms_per_reading=total / n)
        if compose:
            t["host_concatenate_ms"] = cat
        return np.stack(Ts), host, s, t, bus

    def go_back(s):
        b = pc()
        prior = s.take_aligned_map()
        ms = MapSession(ctx, prior, params=loc)
        ms.start_go_back(s)
        return prior, ms, 1e3 * (pc() - b), 0

    def compose_back(host):
        b = pc()
        prior = PriorMap(ctx, host)
        ms = MapSession(ctx, prior, params=loc)
        ms.start()
        return prior, ms, 1e3 * (pc() - b), 16 * len(host)

    recs = dict(keep_off=[], keep_on=[], composition=[])
    backs = dict(go_back=[], compose_back=[])
    bus = {}
    ref_T = None
    for k in range(a.warm + a.runs):
        maps = {}
        for name in ("keep_off", "keep_on", "composition"):  # alternating
            T, host, s, t, b = mapping(name == "keep_on", name == "composition")
            assert ref_T is None or np.array_equal(ref_T.view(np.uint32), T.view(np.uint32)), "the forms' corrections differ"
            ref_T = T
            bus[name] = b
            if name == "keep_on":
                prior, ms, ms_wall, bb = go_back(s)
                bus["go_back"] = bb
                if k >= a.warm:
                    backs["go_back"].append(dict(wall_ms=ms_wall))
                count = ms.state()["count"]
                maps["device"] = prior.getCloud()  # (after the timing: the check's download, not the go-back's)
                ms.close()
                prior.free()
            elif name == "composition":
                prior, ms, ms_wall, bb = compose_back(host)
                bus["compose_back"] = bb
                if k >= a.warm:
                    backs["compose_back"].append(dict(wall_ms=ms_wall))
                maps["host"] = host
                ms.close()
                prior.free()
            s.close()
            if k >= a.warm:
                recs[name].append(t)
        assert maps["device"].shape == maps["host"].shape and \
            np.array_equal(maps["device"].view(np.uint32), maps["host"].view(np.uint32)), "the maps differ"
    out = dict(library=L.build_info(), runs=a.runs, warm=a.warm,
               workload=dict(readings=n, points_per_reading=a.points, reference_update_frequency=5,
                             map_points=int(len(maps["host"])), go_back_count=int(count)),
               variants={v: {k: spread([r[k] for r in recs[v]]) for k in recs[v][0]} for v in recs},
               go_back={v: {k: spread([r[k] for r in backs[v]]) for k in backs[v][0]} for v in backs},
               map_point_bytes_over_the_bus=bus, same_corrections_bit_for_bit=True, same_map_bit_for_bit=True)
    v = out["variants"]
    out["keep_on_over_keep_off_wall"] = (v["keep_on"]["wall_ms_per_reading"]["median"] /
                                         v["keep_off"]["wall_ms_per_reading"]["median"])
    out["keep_on_over_composition_mean_wall"] = (v["keep_on"]["mean_wall_ms_per_reading"]["median"] /
                                                 v["composition"]["mean_wall_ms_per_reading"]["median"])
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
