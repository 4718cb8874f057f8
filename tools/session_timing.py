"""Time the live App session (AppSession, aicp_hip_session_*) against what a caller had before it.

  stream   a C2-size raw stream (64 readings of 120 k points, a reference every 5), reading by reading:
             session_robot / session_debug   AppSession.process per reading (wall: the call on the
                                             host; device: HIP events around its device work)
             run_raw_debug                   aicp_hip_sequence_run_raw in debug mode over the whole
                                             recording: the per-reading mean. It is the session's
                                             reading step driven from C on a session private to the
                                             call, so against session_debug it shows what calling
                                             reading by reading from Python costs, nothing else.
                                             (profiles/session_timing.json records it when it was a
                                             host loop of its own: host reference, a download and a
                                             re-upload per reading.)
             run_raw_robot                   the windowed stream, for scale (it batches readings)
           session_debug and run_raw_debug must give the same bits.
  accum    one reading of 80 sweeps of 32 k points from a SweepAccumulator, from the last push to the
           correction on the host, every reading promoted (frequency 1):
             session       AppSession.process(acc)
             composition   acc.prefilter() to the host, Context.overlap + Context.register of the
                           host arrays, the next reference built on the host
           Both register against structures they have to build (a fresh reference each time).

    python tools/session_timing.py                 # both parts, the variants alternating
    python tools/session_timing.py --part stream

Warmed runs in one process, the variants alternating inside every round; reported per variant: the
median over rounds and the spread (min, max). Writes profiles/session_timing.json (--out).
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

OUT = os.path.join(ROOT, "profiles", "session_timing.json")
pc = time.perf_counter


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=len(v))


def params(L, debug, freq):
    return L.default_sequence_params(reference_update_frequency=freq,
                                     flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))


def part_stream(a, L, ctx):
    from aicp_mapping_amd.session import AppSession

    st = sy.make_stream(n_readings=a.readings, n_points=a.points, seed=1)
    n = a.readings
    sessions = {m: AppSession(ctx, params=params(L, m == "debug", 5), prefilter=True) for m in ("robot", "debug")}

    def run_session(mode):
        s = sessions[mode]
        s.start(st.first, st.first_origin)
        wall, dev, Ts = [], [], []
        t0 = pc()
        for r, o in zip(st.readings, st.origins):
            b = pc()
            T, res, kept = s.process(r, o)
            wall.append(1e3 * (pc() - b))
            dev.append(s.last_timing()["device_ms"])
            Ts.append(T)
        total = 1e3 * (pc() - t0)
        return np.stack(Ts), dict(wall_ms_per_reading=statistics.median(wall), device_ms_per_reading=statistics.median(dev),
                                  mean_wall_ms_per_reading=total / n)

    def run_raw(mode):
        t0 = pc()
        T, out, done, rc = ctx.sequence_run(st.first, st.first_origin, st.readings, st.origins,
                                            params=params(L, mode == "debug", 5), prefilter=True)
        total = 1e3 * (pc() - t0)
        assert rc == 0 and done == n
        return T, dict(mean_wall_ms_per_reading=total / n)

    variants = dict(session_robot=lambda: run_session("robot"), session_debug=lambda: run_session("debug"),
                    run_raw_debug=lambda: run_raw("debug"), run_raw_robot=lambda: run_raw("robot"))
    recs = {k: [] for k in variants}
    Ts = {}
    for k in range(a.warm + a.runs):
        for name, fn in variants.items():  # alternating
            T, t = fn()
            assert name not in Ts or np.array_equal(Ts[name], T), "two runs of one variant differ"
            Ts[name] = T
            if k >= a.warm:
                recs[name].append(t)
    for s in sessions.values():
        s.close()
    out = dict(workload=dict(readings=n, points_per_reading=a.points, reference_update_frequency=5),
               variants={v: {k: spread([r[k] for r in recs[v]]) for k in recs[v][0]} for v in recs})
    out["session_debug_equals_run_raw_debug_bit_for_bit"] = bool(np.array_equal(Ts["session_debug"], Ts["run_raw_debug"]))
    out["session_robot_equals_run_raw_robot_bit_for_bit"] = bool(np.array_equal(Ts["session_robot"], Ts["run_raw_robot"]))
    v = out["variants"]
    out["session_debug_over_run_raw_debug"] = (v["session_debug"]["mean_wall_ms_per_reading"]["median"] /
                                               v["run_raw_debug"]["mean_wall_ms_per_reading"]["median"])
    return out


def sweep_reading(n_sweeps, n_points, x0, seed):
    """A reading as accumulator_timing.py's workload builds it, from poses that start x0 m along."""
    rng = np.random.default_rng(seed * 7919 + 4242)
    w = sy.sample_scene(sy.make_scene(1), rng, (x0, 0.0, 0.7), half=34.0, spacing=0.04)
    total = n_sweeps * n_points
    assert len(w) >= total, (len(w), total)
    w = w[rng.choice(len(w), size=total, replace=False)]
    sweeps, poses = [], []
    for i in range(n_sweeps):
        P = sy.make_T(yaw_deg=0.1 * i, pitch_deg=0.3, roll_deg=-0.2, t=(x0 + 0.02 * i, 0.0, 0.7))
        sweeps.append(sy.transform(np.linalg.inv(P), w[i * n_points:(i + 1) * n_points]))
        poses.append(P)
    return sweeps, poses


def part_accum(a, L, ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator
    from aicp_mapping_amd.session import AppSession

    acc = SweepAccumulator(ctx, a.sweeps * a.sweep_points, batch_size=a.sweeps)

    def fill(sweeps, poses):
        acc.clear()
        for s, P in zip(sweeps, poses):
            acc.push(s, P)

    first_sw, first_poses = sweep_reading(a.sweeps, a.sweep_points, 0.0, 1)
    read_sw, read_poses = sweep_reading(a.sweeps, a.sweep_points, 0.3, 2)
    o0, o1 = first_poses[0][:3, 3].copy(), read_poses[0][:3, 3].copy()
    fill(first_sw, first_poses)
    first_raw = acc.getCloud()
    first_kept = ctx.prefilter(first_raw)
    res = float(np.float32(0.2))
    out = dict(workload=dict(sweeps=a.sweeps, points_per_sweep=a.sweep_points, raw_points=len(first_raw),
                             reference_points=len(first_kept), reference_update_frequency=1), modes={})
    for mode in ("robot", "debug"):
        debug = mode == "debug"
        s = AppSession(ctx, params=params(L, debug, 1), prefilter=True)
        # debug mode needs a non-identity initialT_: one accepted reading before the timed one, whose
        # correction the composition side is given
        warm_sw, warm_poses = sweep_reading(a.sweeps, a.sweep_points, 0.15, 3)
        ow = warm_poses[0][:3, 3].copy()

        def prepare():
            """both sides' state before the timed reading: reference, its origin, initialT_"""
            fill(first_sw, first_poses)
            s.start(acc, o0)
            if not debug:
                return first_kept.copy(), o0, None
            fill(warm_sw, warm_poses)
            s.process(acc, ow)
            ref, org = s.reference()
            return ref, org, s.state()["initial_T"]

        def side_session():
            prepare()
            fill(read_sw, read_poses)
            t0 = pc()
            T, r, kept = s.process(acc, o1)
            t1 = pc()
            return T, kept, dict(last_push_to_correction_ms=1e3 * (t1 - t0), device_ms=s.last_timing()["device_ms"],
                                 **{f"batch_{k}_ms": v for k, v in ctx.last_phase_ms().items()})

        def side_composition():
            ref, org, initT = prepare()
            fill(read_sw, read_poses)
            t0 = pc()
            kept = acc.prefilter(T=initT)
            t1 = pc()
            o = o1 if initT is None else oracle_origin(initT, o1)
            ov = ctx.overlap(ref, kept, org, o, res)
            t2 = pc()
            T, st = ctx.register(ref, kept, L.default_config(trimmed_ratio=L.autotune_ratio(ov)))
            t3 = pc()
            Tf = np.asarray(T, np.float32)
            nxt = (kept @ Tf[:3, :3].T + Tf[:3, 3]).astype(np.float32)  # the next reference, on the host
            t4 = pc()
            assert len(nxt) == len(kept)
            return T, len(kept), dict(last_push_to_correction_ms=1e3 * (t4 - t0), prefilter_ms=1e3 * (t1 - t0),
                                      overlap_ms=1e3 * (t2 - t1), register_ms=1e3 * (t3 - t2), promote_ms=1e3 * (t4 - t3))

        sides = dict(session=side_session, composition=side_composition)
        recs = {k: [] for k in sides}
        last = {}
        for k in range(a.warm + a.runs):
            for name, fn in sides.items():  # alternating
                T, kept, t = fn()
                last[name] = (T, kept)
                if k >= a.warm:
                    recs[name].append(t)
        s.close()
        m = dict(sides={v: {k: spread([r[k] for r in recs[v]]) for k in recs[v][0]} for v in recs},
                 kept_points=int(last["session"][1]),
                 same_results=bool(np.array_equal(last["session"][0], last["composition"][0]) and
                                   last["session"][1] == last["composition"][1]))
        m["session_over_composition"] = (m["sides"]["session"]["last_push_to_correction_ms"]["median"] /
                                         m["sides"]["composition"]["last_push_to_correction_ms"]["median"])
        out["modes"][mode] = m
    acc.free()
    return out


def oracle_origin(T, o):
    """translation of fromMatrix4fToIsometry3d(T) * prior pose (oracle/pyoracle.py: corrected_origin)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle

    return pyoracle.corrected_origin(T, o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("both", "stream", "accum"), default="both")
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--sweeps", type=int, default=80)
    ap.add_argument("--sweep-points", type=int, default=32000)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L

    ctx = L.Context(0)
    rec = dict(library=L.build_info(), runs=a.runs, warm=a.warm)
    if a.part in ("both", "stream"):
        rec["stream"] = part_stream(a, L, ctx)
    if a.part in ("both", "accum"):
        rec["accum"] = part_accum(a, L, ctx)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
