"""Time one aicp_hip_align_chain_batch call against the loop of aicp_hip_register_chain calls it
replaces (reference cache off), for Besl92_pt2point.yaml and icp_3D_cfg_trimmed.yaml
(tests/golden/chains) on two shapes:

  independent  64 pairs of 60 k points a side, every pair with arrays of its own
  all_pairs    8 references x 8 readings of 60 k points: 64 pairs, each reference array shared by 8

The clouds come from 8 synthetic.make_pair scenes; the 64 independent pairs are copies of them in
arrays of their own (no two pairs share a pointer). One process measures both sides, alternating
call by call; after --warm unrecorded rounds the medians of --runs rounds are written, with the kept
counts and whether every pair's transform has the same bits on both sides.

    timeout -k 10 900 python tools/chain_batch_timing.py --out profiles/chain_batch_timing.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_batch_timing.json"))
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--chains", default="Besl92_pt2point,icp_3D_cfg_trimmed")
    a = ap.parse_args()
    f32 = np.float32
    scenes = [sy.make_pair(a.points, a.points, seed=s + 1) for s in range(a.scenes)]
    refs = [np.ascontiguousarray(p.ref, f32) for p in scenes]
    reads = [np.ascontiguousarray(p.read, f32) for p in scenes]
    n = a.scenes
    shapes = dict(
        independent=[dict(ref=refs[k % n].copy(), read=reads[k % n].copy()) for k in range(n * n)],
        all_pairs=[dict(ref=refs[r], read=reads[d]) for r in range(n) for d in range(n)])
    import aicp_mapping_amd._lib as L

    ctx = L.Context(0)
    ctx.set_options(reference_cache=0)
    out = dict(workload=dict(points=a.points, scenes=a.scenes, pairs=n * n, reference_cache=0), library=L.build_info(),
               warm=a.warm, runs=a.runs, order="align_chain_batch, register_chain loop alternating", results={})
    for name in a.chains.split(","):
        rc, cfg, chain = L.parse_pm_chain(os.path.join(ROOT, "tests", "golden", "chains", name + ".yaml"))
        assert rc == 0, rc
        for shape, pairs in shapes.items():
            def batch():
                T, st, cs, rc_ = ctx.align_chain_batch(pairs, cfg, chain, raise_on_error=False)
                return ([t.tobytes() for t in T], [s["status"] for s in st], [c["n_kept"] for c in cs],
                        [s["iterations"] for s in st], [s["converged"] for s in st])

            def loop():
                Ts, sts, kept, its, conv = [], [], [], [], []
                for p in pairs:
                    T, st, cs, rc_ = ctx.register_chain(p["ref"], p["read"], cfg, chain, raise_on_error=False)
                    Ts.append(T.tobytes())
                    sts.append(st["status"])
                    kept.append(cs["n_kept"])
                    its.append(st["iterations"])
                    conv.append(st["converged"])
                return Ts, sts, kept, its, conv

            sides = dict(align_chain_batch=batch, register_chain_loop=loop)
            wall = {k: [] for k in sides}
            last = {}
            for i in range(a.warm + a.runs):
                for k, fn in sides.items():
                    t0 = time.perf_counter()
                    r = fn()
                    dt = 1e3 * (time.perf_counter() - t0)
                    assert last.get(k) is None or last[k][0] == r[0], f"two {k} rounds differ"
                    last[k] = r
                    if i >= a.warm:
                        wall[k].append(dt)
            b, l = last["align_chain_batch"], last["register_chain_loop"]
            same = [x == y for x, y in zip(b[0], l[0])]
            res = dict(pairs=len(pairs), distinct_references=len({id(p["ref"]) for p in pairs}),
                       transforms_bit_equal=bool(all(same)), pairs_bit_equal=int(sum(same)),
                       statuses_equal=bool(b[1] == l[1]), kept_equal=bool(b[2] == l[2]),
                       statuses=sorted(set(b[1])), iterations_equal=bool(b[3] == l[3]),
                       iterations_total=int(sum(b[3])), iterations_max=int(max(b[3])), converged_pairs=int(sum(b[4])),
                       kept_first_pair=[int(v) for v in b[2][0]],
                       kept_total=[int(sum(k[0] for k in b[2])), int(sum(k[1] for k in b[2]))], sides={})
            for k in sides:
                res["sides"][k] = dict(wall_ms=dict(median=statistics.median(wall[k]), min=min(wall[k]), max=max(wall[k]),
                                                    all=[round(v, 3) for v in wall[k]]),
                                       per_pair_ms=statistics.median(wall[k]) / len(pairs))
            res["batch_over_loop_wall"] = res["sides"]["align_chain_batch"]["wall_ms"]["median"] / \
                res["sides"]["register_chain_loop"]["wall_ms"]["median"]
            out["results"][f"{name}/{shape}"] = res
            print(name, shape, json.dumps(res["sides"]), res["batch_over_loop_wall"], res["transforms_bit_equal"], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["workload"]))


if __name__ == "__main__":
    main()
