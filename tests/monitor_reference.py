"""Restatement of the registration quality monitor (aicp_core/src/utils/icpMonitor.cpp) on the CPU
oracle: hausdorffDistance (:12-81), distancesKNN (:89-138) and pairedPointsMeanDistance (:146-231,
with the matcher's own d2). Test infrastructure only.

Every piece is the oracle's: transform_cloud (pcl::transformPointCloud in float), Tree(pts).knn
(libnabo order; epsilon as KDTreeMatcher passes it), dists_quantile (Matches::getDistsQuantile),
np.sqrt on float32 (correctly rounded, as sqrtf) and math.fsum for the two sums, so the means are
the correctly rounded quotients of the exact sums.
"""
import math

import numpy as np


def quantile_index(n, q):
    """The element Matches::getDistsQuantile returns from the n sorted finite values:
    values[(size_t)((float)n * q)], and the last one for q == 1."""
    if np.float32(q) == np.float32(1.0):
        return n - 1
    return min(int(np.float32(n) * np.float32(q)), n - 1)


def mean_f32(values):
    """float32 of the exact sum over the count; NaN for no value (the reference divides 0 by 0)."""
    if len(values) == 0:
        return np.float32(np.nan)
    return np.float32(math.fsum(float(v) for v in values) / len(values))


def monitor(oracle, ref, out, T=None, quantile=0.6, max_accepted_dist=0.2, cfg=None):
    """The aicp_monitor_result fields (plus d2_out / d2_ref / dist_out / dist_ref) for the reference
    cloud and the aligned reading; with T (4x4 row-major) out = transform_cloud(T, out). cfg (an
    IcpConfig of either binding): the chain matcher's paired mean as well."""
    ref = np.ascontiguousarray(np.asarray(ref, np.float32)[:, :3])
    out = np.ascontiguousarray(np.asarray(out, np.float32)[:, :3])
    if T is not None:
        out = oracle.transform_cloud(T, out)
    d2 = [oracle.Tree(ref).knn(out, k=1, eps=0.0)[1][:, 0].copy(),   # [0] tree on ref, queries from out
          oracle.Tree(out).knn(ref, k=1, eps=0.0)[1][:, 0].copy()]   # [1] tree on out, queries from ref
    r = {}
    r["max_d2"], r["quantile_d2"] = [], []
    for d in d2:
        mx, e1 = oracle.dists_quantile(d, 1.0)
        qv, e2 = oracle.dists_quantile(d, float(np.float32(quantile)))
        assert e1 == 0 and e2 == 0
        r["max_d2"].append(np.float32(mx))
        r["quantile_d2"].append(np.float32(qv))
    r["hausdorff"] = np.sqrt(np.float32(max(r["max_d2"])))
    r["hausdorff_quantile"] = np.sqrt(np.float32(max(r["quantile_d2"])))
    dist = [np.sqrt(d) for d in d2]
    valid = dist[0].astype(np.float64) <= float(max_accepted_dist)
    r["knn_valid"] = int(valid.sum())
    r["knn_mean_dist"] = mean_f32(dist[0][valid])
    r["paired_mean_dist"], r["paired_limit_d2"], r["paired_kept"] = np.float32(np.nan), np.float32(np.nan), 0
    if cfg is not None:
        eps, md = float(cfg.nn_epsilon), float(cfg.nn_max_dist)
        if eps == 0.0 and math.isinf(md) and cfg.bucket_size == 8:
            dp = d2[0]
        else:
            dp = oracle.Tree(ref, bucket=cfg.bucket_size).knn(out, k=1, eps=eps, max_radius=md)[1][:, 0].copy()
        lim, err = oracle.dists_quantile(dp, float(cfg.trimmed_ratio))
        if err == 0:
            kept = dp <= np.float32(lim)
            r["paired_limit_d2"] = np.float32(lim)
            r["paired_kept"] = int(kept.sum())
            r["paired_mean_dist"] = mean_f32(np.sqrt(dp[kept]))
        r["d2_paired"] = dp
    r["d2_out"], r["d2_ref"] = d2
    r["dist_out"], r["dist_ref"] = dist
    return r
