"""Time the quality monitor per reading in the live App session against what a caller had before it.

A C2-size raw stream (64 readings of 120 k points, a reference every 5; tools/session_timing.py's),
reading by reading through AppSession.process, in robot and in debug mode. Three variants, in one
process, alternating round by round:

  monitor_on    the session with monitor=True: the resident monitor runs behind the registration
  monitor_off   the session without it
  composed      monitor_off plus, per reading, what a caller had to do for the same 56 bytes:
                session.reference() downloaded before the call, the registered reading rebuilt with
                ctx.prefilter (after ctx.transform by initialT_ in debug mode), and ctx.monitor

Per variant and round: the median over the readings of the call's wall time (composed: the call and
the composition) and of the session's device time; reported: the median over rounds with (min, max).
monitor_on - monitor_off and composed - monitor_off are taken round by round. monitor_on and composed
must give the same 56 bytes per reading. Writes profiles/session_monitor_timing.json (--out).

    python tools/session_monitor_timing.py
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

OUT = os.path.join(ROOT, "profiles", "session_monitor_timing.json")
pc = time.perf_counter


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=len(v))


def params(L, debug, freq):
    return L.default_sequence_params(reference_update_frequency=freq,
                                     flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))


def run_mode(a, L, ctx, st, debug):
    from aicp_mapping_amd.session import AppSession

    sessions = dict(monitor_on=AppSession(ctx, params=params(L, debug, a.freq), prefilter=True, monitor=True),
                    monitor_off=AppSession(ctx, params=params(L, debug, a.freq), prefilter=True))

    def run(variant):
        composed = variant == "composed"
        s = sessions["monitor_off" if composed else variant]
        s.start(st.first, st.first_origin)
        wall, dev, mon, Ts = [], [], [], []
        for r, o in zip(st.readings, st.origins):
            b = pc()
            if composed:
                ref = s.reference()[0]
                initT = s.state()["initial_T"]
            T, res, kept = s.process(r, o)
            if composed:
                reg = ctx.prefilter(ctx.transform(initT, r) if debug else r)
                mon.append(ctx.monitor(ref, reg, T)["bytes"])
            wall.append(1e3 * (pc() - b))
            dev.append(s.last_timing()["device_ms"])
            if variant == "monitor_on":
                mon.append(s.last_monitor()["bytes"])
            Ts.append(T)
        rec = dict(wall_ms_per_reading=statistics.median(wall), device_ms_per_reading=statistics.median(dev),
                   mean_wall_ms_per_reading=statistics.fmean(wall))
        return np.stack(Ts), mon, rec, (s.monitor_counters() if variant == "monitor_on" else None)

    order = ("monitor_on", "monitor_off", "composed")
    recs = {k: [] for k in order}
    last, counters = {}, None
    for k in range(a.warm + a.runs):
        for name in order:  # alternating
            T, mon, t, c = run(name)
            assert name not in last or np.array_equal(last[name][0], T), "two runs of one variant differ"
            last[name] = (T, mon)
            counters = c or counters
            if k >= a.warm:
                recs[name].append(t)
    for s in sessions.values():
        s.close()
    out = dict(variants={v: {k: spread([r[k] for r in recs[v]]) for k in recs[v][0]} for v in recs})
    for key in ("wall_ms_per_reading", "mean_wall_ms_per_reading", "device_ms_per_reading"):
        off = [r[key] for r in recs["monitor_off"]]
        out[f"monitor_on_minus_off_{key}"] = spread([x[key] - y for x, y in zip(recs["monitor_on"], off)])
        if key != "device_ms_per_reading":  # (the composition's device work lies outside the session's events)
            out[f"composed_minus_off_{key}"] = spread([x[key] - y for x, y in zip(recs["composed"], off)])
    out["same_T_bit_for_bit"] = bool(np.array_equal(last["monitor_on"][0], last["monitor_off"][0]) and
                                     np.array_equal(last["monitor_on"][0], last["composed"][0]))
    out["same_monitor_bytes"] = last["monitor_on"][1] == last["composed"][1]
    out["counters_of_all_rounds"] = counters  # (a session keeps counting across start())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--freq", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L

    ctx = L.Context(0)
    st = sy.make_stream(n_readings=a.readings, n_points=a.points, seed=1)
    rec = dict(library=L.build_info(), runs=a.runs, warm=a.warm,
               workload=dict(readings=a.readings, points_per_reading=a.points, reference_update_frequency=a.freq),
               modes={m: run_mode(a, L, ctx, st, m == "debug") for m in ("robot", "debug")})
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
