"""Stage times of aicp_hip_alignment_features on two C2-size raw clouds (the `bench.py --config
prefilter` generator: half 25 m, spacing 0.035 m, about 2.4 M points each), beside what the two
pre-filters alone cost on the same accepted clouds (two aicp_hip_prefilter calls, the part the
library already had).

    python tools/risk_timing.py [--reps 10] [--warmup 3] [--view 270] [--range 100] [--out FILE]

Prints one JSON line: medians over the repetitions of aicp_hip_last_risk_stats and of the two
aicp_hip_last_prefilter_stats device times, and `added_ms` = device_ms - their sum.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import aicp_mapping_amd._lib as L  # noqa: E402
from aicp_mapping_amd import synthetic as sy  # noqa: E402


def raw_clouds(half, spacing, seed=1):
    scene = sy.make_scene(seed)
    origins = [np.array([0.0, 0.0, 0.7]), np.array([0.3, 0.0, 0.7])]
    clouds = [sy.sample_scene(scene, np.random.default_rng(seed * 1000 + i), o, half=half,
                              spacing=spacing).astype(np.float32) for i, o in enumerate(origins)]
    return clouds, origins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--view", type=float, default=270.0)
    ap.add_argument("--range", type=float, default=100.0)
    ap.add_argument("--half", type=float, default=25.0)
    ap.add_argument("--spacing", type=float, default=0.035)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    (A, B), (oa, ob) = raw_clouds(a.half, a.spacing)
    pa, pb = np.eye(4), np.eye(4)
    pa[:3, 3], pb[:3, 3] = oa, ob
    prm = L.default_risk_params(range=a.range, angular_view=a.view)
    ctx = L.Context(0)
    _, ka, kb = ctx.fov_overlap(A, B, pa, pb, a.range, a.view)
    pfa = L.default_prefilter(viewpoint=tuple(np.float32(oa)))
    pfb = L.default_prefilter(viewpoint=tuple(np.float32(ob)))
    rows, pf_rows, res = [], [], None
    for i in range(a.warmup + a.reps):
        res = ctx.alignment_features(A, B, pa, pb, prm)
        st = ctx.last_risk_stats()
        ctx.prefilter(ka, pfa)
        da = ctx.last_prefilter_stats()["device_ms"]
        ctx.prefilter(kb, pfb)
        db = ctx.last_prefilter_stats()["device_ms"]
        if i >= a.warmup:
            rows.append(st)
            pf_rows.append(da + db)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    pf = float(np.median(pf_rows))
    out = {
        "tool": "tools/risk_timing.py", "library": L.provenance()["build_info"],
        "points": [len(A), len(B)], "accepted": [int(res["accepted_a"]), int(res["accepted_b"])],
        "sampled": [int(res["sampled_a"]), int(res["sampled_b"])],
        "clusters": [int(res["clusters_a"]), int(res["clusters_b"])], "n_matches": int(res["n_matches"]),
        "fov_overlap": float(res["fov_overlap"]), "alignability": float(res["alignability"]),
        "view": a.view, "range": a.range, "reps": a.reps, "warmup": a.warmup,
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_device_ms": round(min(r["device_ms"] for r in rows), 4),
        "max_device_ms": round(max(r["device_ms"] for r in rows), 4),
        "two_prefilters_device_ms": round(pf, 4),
        "added_ms": round(med["device_ms"] - pf, 4),
        "new_kernels_ms": round(med["fov_ms"] + med["clusters_ms"] + med["counts_ms"] + med["match_ms"], 4),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
