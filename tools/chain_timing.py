"""Time aicp_hip_register_chain on a sampled chain against the composition a caller had before it:
aicp_hip_chain_filter of each side with the kept indices downloaded, the two filtered clouds gathered
on the host, then aicp_hip_register on them (reference cache off).

A C2-size pair (120 k points a side, synthetic.make_pair) through the icp_3D_cfg_trimmed.yaml chain
(tests/golden/chains): reference SurfaceNormal knn 10 -> RandomSampling 0.5, reading SurfaceNormal
knn 10 with densities -> MaxDensity 50, TrimmedDist 0.75, point-to-plane. For this chain the
composition is NOT the same computation: it recomputes the reference's normals on the sampled
subset, where the chain carries those of the full cloud (for Besl92's point-to-point chain the two
are the same computation; --chain Besl92_pt2point times that one, and the transforms are compared).

One process measures both, alternating call by call; after --warm unrecorded calls of each the
medians of --runs calls are written, as tools/p2p_timing.py does.

    timeout -k 10 300 python tools/chain_timing.py --out profiles/chain_timing.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_timing.json"))
    ap.add_argument("--chain", default="icp_3D_cfg_trimmed")
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    pr = sy.make_pair(a.points, a.points, seed=a.seed)
    ref, read = np.ascontiguousarray(pr.ref, np.float32), np.ascontiguousarray(pr.read, np.float32)
    import aicp_mapping_amd._lib as L

    rc, cfg, chain = L.parse_pm_chain(os.path.join(ROOT, "tests", "golden", "chains", a.chain + ".yaml"))
    assert rc == 0, rc
    ctx = L.Context(0)
    ctx.set_options(reference_cache=0)

    def fused():
        T, st, cs, _ = ctx.register_chain(ref, read, cfg, chain)
        return T, st, cs["n_kept"]

    def composed():
        fr = ctx.chain_filter(chain, L.AICP_CHAIN_REFERENCE, ref)
        fd = ctx.chain_filter(chain, L.AICP_CHAIN_READING, read)
        T, st = ctx.register(ref[fr["index"]], read[fd["index"]], cfg)
        return T, st, [fr["n"], fd["n"]]

    sides = dict(register_chain=fused, filter_download_register=composed)
    wall = {k: [] for k in sides}
    last = {}
    for i in range(a.warm + a.runs):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            T, st, kept = fn()
            dt = 1e3 * (time.perf_counter() - t0)
            assert last.get(k) is None or last[k][0].tobytes() == T.tobytes(), f"two {k} calls differ"
            last[k] = (T, st, kept)
            if i >= a.warm:
                wall[k].append(dt)
    ctx.close()
    same = last["register_chain"][0].tobytes() == last["filter_download_register"][0].tobytes()
    r, t = sy.rot_err(last["register_chain"][0], last["filter_download_register"][0])
    out = dict(workload=dict(points_ref=int(len(ref)), points_read=int(len(read)), seed=a.seed, reference_cache=0,
                             chain=a.chain, chain_seed=int(chain.seed)),
               library=L.build_info(), warm=a.warm, runs=a.runs,
               order="register_chain, filter_download_register alternating",
               same_computation=bool(cfg.knn_normals == 0),
               note=("point-to-point: both sides compute the same thing" if cfg.knn_normals == 0 else
                     "point-to-plane: the composition recomputes the reference's normals on the sampled subset; "
                     "register_chain carries the full cloud's normals, as libpointmatcher does"),
               transforms_bit_equal=bool(same), transforms_differ_by=dict(rad=r, m=t), sides={})
    for k in sides:
        T, st, kept = last[k]
        out["sides"][k] = dict(
            wall_ms=dict(median=statistics.median(wall[k]), min=min(wall[k]), max=max(wall[k]),
                         all=[round(v, 3) for v in wall[k]]),
            kept=[int(v) for v in kept], iterations=st["iterations"], converged=st["converged"], status=st["status"],
            inlier_ratio=st["inlier_ratio"])
    s = out["sides"]
    out["register_chain_over_composition_wall"] = s["register_chain"]["wall_ms"]["median"] / \
        s["filter_download_register"]["wall_ms"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
