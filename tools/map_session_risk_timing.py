#!/usr/bin/env python3
"""Per-reading time of failure_prediction_mode served in the live map sessions (MapSession(...,
risk=...): aicp_hip_mapsession_create_risk) against the composition a node had to write before it,
on the workload of tools/map_session_timing.py: a resident 1 M-point map (built map: a 120 k-point
first cloud), 64 raw readings of about 277 k points, crop -15..15, a merge / reference every 5
accepted readings, a re-filter every 30 (prior map), octree 0.2 m (built map). The golden opencv3
model under threshold 0.0 (every reading gated) and 1.0 (none).

The composition keeps its map on the device too and applies the rules of include/aicp_hip.h from the
public one-reading calls: ctx.prefilter (kept points down), map.crop (the crop down), the one-pair
overlap (crop and reading up; built map), ctx.alignment_features (both up again), ctx.svm_predict,
the map's one-reading registration (the reading up a third time), map.merge / map.prefilter.

Both policies and both working modes in one process; inside every round the session and the
composition alternate, each on a fresh copy of the map made outside the timed region. Bit equality
(corrections, decisions, counts, records) and the final maps are checked on the warm-up round
before anything is timed; then the medians of --runs rounds with (min, max), in milliseconds per
reading, go to profiles/map_session_risk_timing.json with what crossed the bus for the median
reading, listed from the code paths (they are not traced).

    python tools/map_session_risk_timing.py [--out profiles/map_session_risk_timing.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raw_localization_timing as rl  # noqa: E402  (the workload, unchanged)
import map_session_risk_reference as mr  # noqa: E402  (MapGatePolicy: the rules' bookkeeping)
import svm_reference as sr  # noqa: E402  (the golden model's path, the poses)

FREQ, REFILTER, MAX_CORR, CROP, RES = rl.FREQ, rl.REFILTER, rl.MAX_CORR, rl.CROP, rl.RES
F32 = np.float32


def crossings(policy, n_raw, kept, crop, gated):
    """Point data over the bus for one reading (bytes), from the code paths; control blocks,
    descriptors and records (a few hundred bytes each) are left out."""
    built = policy == "built"
    session = [("H2D", n_raw * 12, "the reading's raw rows (0 from a sweep accumulator)")]
    comp = [("H2D", n_raw * 12, "ctx.prefilter: the raw rows"), ("D2H", kept * 12, "ctx.prefilter: the kept points"),
            ("D2H", crop * 12, "map.crop: the crop")]
    if built:
        comp.append(("H2D", (crop + kept) * 16, "one-pair overlap: crop and reading"))
    comp.append(("H2D", (crop + kept) * 16, "alignment_features: crop and reading"))
    if gated:
        if built:
            comp.append(("H2D", kept * 16, "map.merge: the reading"))
    else:
        comp.append(("H2D", kept * 16, "the map's registration: the reading"))
        comp.append(("H2D", "kept * 16 when it appends", "map.merge: the reading"))
    total = lambda rows: int(sum(b for _, b, _ in rows if isinstance(b, int)))  # noqa: E731
    return dict(session_bytes=total(session), composition_bytes=total(comp))  # (the rows above say what they are)


def measure(L, ctx, policy, mp, raws, poses, model, thr, debug, rp, warm, runs):
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.prior_map import PriorMap

    built = policy == "built"
    cls, append = (BuiltMap, "is_reference") if built else (PriorMap, "merged")
    n = len(raws)
    if built:
        prm = L.default_built_map_params(reference_update_frequency=FREQ, max_correction_magnitude=MAX_CORR,
                                         crop_min=-CROP, crop_max=CROP, resolution=RES, debug=debug)
    else:
        prm = L.default_localization_params(reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                                            max_correction_magnitude=MAX_CORR, crop_min=-CROP, crop_max=CROP,
                                            debug=debug)
    cfg = L.default_config()

    def session_side():
        m = cls(ctx, mp)
        s = MapSession(ctx, m, params=prm, prefilter=True, risk=dict(model=model, threshold=thr, params=rp))
        s.start()
        rows = []
        t0 = time.perf_counter()
        for r, P in zip(raws, poses):
            T, d, k, rec = s.process(r, P)
            rows.append(dict(T=T, registered=rec["registered"], accepted=d["accepted"], append=d[append],
                             refilter=d.get("refiltered", 0), kept=k, crop=d["crop_points"], map=d["map_points"],
                             iterations=d["icp"]["iterations"], raw=rec["raw"], risk=rec["risk"],
                             overlap=rec["octree_overlap"], alignability=rec["alignability"],
                             fov=rec["fov_overlap"], ratio=rec["trimmed_ratio"]))
        dt = 1e3 * (time.perf_counter() - t0)
        final = m.getCloud()
        s.close()
        m.free()
        return dt / n, rows, final

    def composed_side():
        m = cls(ctx, mp)
        policy_ = mr.MapGatePolicy(built, FREQ, MAX_CORR, thr, REFILTER if not built else 0, True)
        rows = []
        t0 = time.perf_counter()
        for r, pose in zip(raws, poses):
            P = np.asarray(pose, np.float64).reshape(4, 4)
            P32 = P.astype(F32)
            prior = sr.moved_pose(policy_.initT, P) if debug else P
            rd = ctx.prefilter(ctx.transform(policy_.initT, r) if debug else r)
            n_map = len(m)
            crop = m.crop(-CROP, CROP, P32)
            ov = 50.0
            if built:
                _, st, rc = ctx.align_batch([dict(ref=crop, read=rd, ref_origin=P32[:3, 3].astype(np.float64),
                                                  read_origin=prior[:3, 3])], flags=L.AICP_RUN_OVERLAP, resolution=RES)
                ov = st[0]["overlap_percent"]
            f = ctx.alignment_features(crop, rd, P, prior, rp)
            raw, risk = ctx.svm_predict(model, np.array([[ov, f["alignability"]]], F32))
            ratio = L.autotune_ratio(float(F32(ov)))
            T, iters = np.eye(4, dtype=F32), 0
            if not policy_.gated(risk[0]):
                if built:
                    c = type(cfg).from_buffer_copy(cfg)
                    c.trimmed_ratio = ratio
                    Ts, st, rc = m.align_batch([rd], [P32], -CROP, CROP, cfg=c, flags=0)
                else:
                    Ts, st, rc = m.register_batch([rd], [P32], -CROP, CROP, cfg=cfg)
                T, iters = Ts[0], st[0]["iterations"]
            d = policy_.step(risk[0], T)
            if d["append"]:  # (a gated reading by the identity: only a -0.0f would differ from its bytes)
                m.merge(rd, T)
            if d["refilter"]:
                m.prefilter()
            rows.append(dict(T=np.asarray(T, F32), registered=d["registered"], accepted=d["accepted"],
                             append=d["append"], refilter=d["refilter"], kept=len(rd), crop=len(crop), map=n_map,
                             iterations=iters, raw=float(raw[0]), risk=float(risk[0]), overlap=float(F32(ov)),
                             alignability=float(F32(f["alignability"])), fov=float(F32(f["fov_overlap"])),
                             ratio=float(F32(ratio))))
        dt = 1e3 * (time.perf_counter() - t0)
        final = m.getCloud()
        m.free()
        return dt / n, rows, final

    ts = dict(session=[], composition=[])
    rows = None
    for k in range(warm + runs):
        order = (("session", session_side), ("composition", composed_side))
        got = {}
        for name, fn in (order if k % 2 == 0 else order[::-1]):
            got[name] = fn()
            if k >= warm:
                ts[name].append(got[name][0])
        if k == 0:  # bit equality first
            (_, a, fa), (_, b, fb) = got["session"], got["composition"]
            for i, (x, y) in enumerate(zip(a, b)):
                assert x["T"].tobytes() == y["T"].tobytes(), ("T", i)
                for key in x:
                    if key != "T":
                        assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), (key, i, x[key], y[key])
            assert fa.shape == fb.shape and np.array_equal(fa, fb), "final maps differ"
            rows = a
    kept = [r["kept"] for r in rows]
    med = int(np.argsort(kept)[len(kept) // 2])
    out = dict(policy=policy, mode="debug" if debug else "robot", threshold=thr,
               gated=int(sum(1 - r["registered"] for r in rows)), accepted=int(sum(r["accepted"] for r in rows)),
               appended=int(sum(r["append"] for r in rows)), refiltered=int(sum(r["refilter"] for r in rows)),
               kept_median=kept[med], crop_median=int(statistics.median(r["crop"] for r in rows)),
               session_equals_composition_bit_for_bit=True,
               session_ms_per_reading=rl.spread(ts["session"]), composition_ms_per_reading=rl.spread(ts["composition"]),
               bus_of_the_median_reading=crossings(policy, len(raws[med]), kept[med], rows[med]["crop"],
                                                   not rows[med]["registered"]))
    out["composition_over_session"] = (out["composition_ms_per_reading"]["median_ms"] /
                                       out["session_ms_per_reading"]["median_ms"])
    return out


def dump(out, path):
    """The result as JSON, one line per case."""
    head = {k: v for k, v in out.items() if k != "cases"}
    with open(path, "w") as f:
        f.write(json.dumps(head)[:-1] + ', "cases": [\n' + ",\n".join(json.dumps(c) for c in out["cases"]) + "\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_session_risk_timing.json"))
    ap.add_argument("--map", type=int, default=1000000)
    ap.add_argument("--first", type=int, default=120000)
    ap.add_argument("--readings", type=int, default=64)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--policies", nargs="+", default=["prior", "built"])
    a = ap.parse_args()
    import aicp_mapping_amd._lib as L

    raws, poses = rl.workload(a.readings)
    ctx = L.Context(0)
    model = L.SvmModel(os.path.join(sr.GOLDEN, sr.MODELS["opencv3"][0]))
    rp = L.default_risk_params(angular_view=270.0)
    out = dict(library=L.build_info(), runs=a.runs, warm=a.warm, unit="ms per reading",
               workload=dict(readings=len(raws), raw_points_median=int(statistics.median(len(r) for r in raws)),
                             crop=CROP, reference_update_frequency=FREQ, map_refilter_every=REFILTER,
                             max_correction_magnitude=MAX_CORR, resolution=RES, model=sr.MODELS["opencv3"][0], view=270.0),
               cases=[])
    maps = dict(prior=rl._map(a.map))
    if "built" in a.policies:
        maps["built"] = ctx.prefilter(rl._first(a.first))  # App's first cloud, pre-filtered
    for policy in a.policies:
        for debug in (False, True):
            for thr in (0.0, 1.0):
                c = measure(L, ctx, policy, maps[policy], raws, poses, model, thr, debug, rp, a.warm, a.runs)
                out["cases"].append(c)
                print(json.dumps({k: v for k, v in c.items() if k != "bus_of_the_median_reading"}), flush=True)
                dump(out, a.out)  # (kept after every case: a run that is cut short leaves its part)
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
