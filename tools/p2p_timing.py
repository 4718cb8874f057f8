"""Time aicp_hip_register with the point-to-point minimizer against the point-to-plane one on the
same pair: a C2-size pair (120 k points a side, synthetic.make_pair), the default chain with only
the minimizer changed (default_config(point_to_point=True)), the reference cache off so every call
builds its trees (and, for point-to-plane, the raw tree, the normals' kNN and the scatter).

One process measures both, alternating call by call; after --warm unrecorded calls of each the
medians of --runs calls are written with the per-phase times of aicp_hip_last_phase_ms (overlap,
reference normals chain, matcher tree, ICP loop, host total) and both iteration counts.

Every GPU step under a time limit of its own, chained:

    timeout -k 10 300 python tools/p2p_timing.py --out profiles/p2p_timing.json && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d OUT -- python tools/p2p_timing.py --warm 1 --runs 3 --out OUT/t.json

(the second for the kernels' own times: k_icp_reduce_p2p beside k_icp_reduce).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2p_timing.json"))
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    pr = sy.make_pair(a.points, a.points, seed=a.seed)
    ref, read = np.ascontiguousarray(pr.ref, np.float32), np.ascontiguousarray(pr.read, np.float32)
    import aicp_mapping_amd._lib as L

    ctx = L.Context(0)
    ctx.set_options(reference_cache=0)
    cfgs = dict(point_to_plane=L.default_config(), point_to_point=L.default_config(point_to_point=True))
    wall = {k: [] for k in cfgs}
    phases = {k: [] for k in cfgs}
    last = {}
    for i in range(a.warm + a.runs):
        for k, cfg in cfgs.items():
            t0 = time.perf_counter()
            T, st = ctx.register(ref, read, cfg)
            dt = 1e3 * (time.perf_counter() - t0)
            assert last.get(k) is None or last[k][0].tobytes() == T.tobytes(), f"two {k} calls differ"
            last[k] = (T, st)
            if i >= a.warm:
                wall[k].append(dt)
                phases[k].append(ctx.last_phase_ms())
    ctx.close()
    out = dict(workload=dict(points_ref=int(len(ref)), points_read=int(len(read)), seed=a.seed, reference_cache=0,
                             chain="default (eps 3.16, ratio 0.70, Counter 20, Differential 1e-3 / 1e-2 / 4)"),
               library=L.build_info(), warm=a.warm, runs=a.runs, order="point_to_plane, point_to_point alternating",
               sides={})
    for k in cfgs:
        T, st = last[k]
        out["sides"][k] = dict(
            wall_ms=dict(median=statistics.median(wall[k]), min=min(wall[k]), max=max(wall[k]),
                         all=[round(v, 3) for v in wall[k]]),
            phases_ms={p: statistics.median(ph[p] for ph in phases[k]) for p in phases[k][0]},
            iterations=st["iterations"], converged=st["converged"], status=st["status"],
            inlier_ratio=st["inlier_ratio"])
    s = out["sides"]
    out["point_to_point_over_point_to_plane_wall"] = s["point_to_point"]["wall_ms"]["median"] / \
        s["point_to_plane"]["wall_ms"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
