"""Time the registration quality monitor on a C2-size pair (120k points a side) against the
composition of kernel-level calls that offered the same numbers before it: aicp_hip_transform, two
aicp_hip_knn, four aicp_hip_dists_quantile and numpy. Medians of 10 warmed calls; writes
profiles/monitor_timing.json.

    python tools/monitor_timing.py [points] [calls]
"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicp_mapping_amd import synthetic as sy  # noqa: E402
import aicp_mapping_amd._lib as L  # noqa: E402


def composition(ctx, ref, cloud, T, quantile=0.6, max_accepted=0.2):
    """The monitor's Hausdorff and kNN-mean numbers from the kernel-level entry points."""
    out = ctx.transform(T, cloud)
    d0 = ctx.knn(ref, out, k=1)[1][:, 0]
    d1 = ctx.knn(out, ref, k=1)[1][:, 0]
    mx = [ctx.dists_quantile(d, 1.0) for d in (d0, d1)]
    qv = [ctx.dists_quantile(d, quantile) for d in (d0, d1)]
    dist = np.sqrt(d0)
    valid = dist.astype(np.float64) <= max_accepted
    mean = np.float32(math.fsum(dist[valid].astype(np.float64)) / valid.sum()) if valid.any() else np.float32(np.nan)
    return dict(hausdorff=float(np.sqrt(np.float32(max(mx)))), hausdorff_quantile=float(np.sqrt(np.float32(max(qv)))),
                max_d2=[float(v) for v in mx], quantile_d2=[float(v) for v in qv], knn_valid=int(valid.sum()),
                knn_mean_dist=float(mean))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 120000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    pr = sy.make_pair(n, n, seed=3)
    ctx = L.Context(0)
    cfg = L.default_config()
    T, st = ctx.register(pr.ref, pr.read, cfg)
    runs = {"monitor": lambda: ctx.monitor(pr.ref, pr.read, T=T),
            "monitor_paired": lambda: ctx.monitor(pr.ref, pr.read, T=T, cfg=cfg),
            "composition": lambda: composition(ctx, pr.ref, pr.read, T)}
    wall, phases, values = {}, {}, {}
    for name, fn in runs.items():
        for _ in range(3):
            values[name] = fn()
        ts, ph = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
            if name != "composition":
                ph.append(ctx.last_monitor_stats())
        wall[name] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
        if ph:
            phases[name] = {k: statistics.median(p[k] for p in ph) for k in ph[0]}
    m, c = values["monitor"], values["composition"]
    same = all(np.float32(m[k]) == np.float32(c[k]) for k in ("hausdorff", "hausdorff_quantile", "knn_mean_dist")) and \
        m["max_d2"] == c["max_d2"] and m["quantile_d2"] == c["quantile_d2"] and m["knn_valid"] == c["knn_valid"]
    rec = dict(points=[len(pr.ref), len(pr.read)], calls=calls, iterations=st["iterations"], wall_ms=wall,
               phases_ms=phases, same_values_as_composition=bool(same),
               values={k: v for k, v in values["monitor_paired"].items() if k != "bytes"}, library=L.build_info())
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "monitor_timing.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
