"""Host mirror of aicp_core's pre-filter (aicp_core/include/aicp_utils/filteringUtils.hpp:29-34,
aicp_core/src/utils/filteringUtils.cpp:5-103), SURVEY.md §8(f) rank 2.

Both overloads run on the device through aicp_hip_prefilter (kernels_prefilter.hip):
VoxelGrid 0.08 -> NormalEstimation k = 30 -> RegionGrowing (15 neighbours, 3 deg smoothness,
curvature 1.0, clusters of 50..1e6 points). There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_CTX = None


def _ctx(ctx):
    global _CTX
    if ctx is not None:
        return ctx
    if _CTX is None:
        _CTX = _lib.Context(0)
    return _CTX


def _cluster_rgb(c: int) -> float:
    """Colour of cluster c as the reference stores it: ``points[idx].rgb = rgb`` with an int32
    ``rgb = (r << 16) | (g << 8) | b`` (filteringUtils.cpp:92-100) is a numeric int -> float
    conversion of the float field, not a bit-packed colour, and so it is here. The reference draws
    r, g, b at random (srand(time(NULL)), :89); a fixed hash of the cluster index here, so runs
    are repeatable."""
    h = (c * 2654435761 + 12345) & 0xFFFFFFFF
    rgb = ((h >> 8) & 0xFF) << 16 | ((h >> 16) & 0xFF) << 8 | ((h >> 24) & 0xFF)
    return float(np.float32(rgb))


def regionGrowingUniformPlaneSegmentationFilter(cloud_in, *args, ctx=None, params=None):
    """filteringUtils.cpp overloads, as in the reference:

    - ``regionGrowingUniformPlaneSegmentationFilter(cloud_in[, cloud_out])`` (:5-45): returns the
      points of the kept plane clusters, clusters concatenated in creation order, each in
      sampled-cloud order, appended to ``cloud_out`` when given (``*cloud_out = *cloud_out +
      cloud_cluster``).
    - ``regionGrowingUniformPlaneSegmentationFilter(cloud_in, view_point, clusters)`` (:51-103,
      view_point a 4x4 pose, clusters a list to fill like ``std::vector<pcl::PointIndices>&``):
      returns the sampled cloud as (V, 12) PointXYZRGBNormal rows {x, y, z, 1, nx, ny, nz, 0,
      rgb, curvature, 0, 0}; normals face view_point.translation(); each kept cluster's points
      carry one colour (rgb = float(int32 colour), the reference's numeric conversion).

    cloud_in: (N, 3|4|8|12) float32 rows. ctx: an aicp Context (default: one on device 0)."""
    if len(args) > 2:
        raise TypeError("expected (cloud_in[, cloud_out]) or (cloud_in, view_point, clusters)")
    c = _ctx(ctx)
    if len(args) == 2:
        view_point, clusters = args
        T = np.asarray(view_point, np.float64).reshape(4, 4)
        # a copy: the caller's params keep their own viewpoint (the first overload's is (0,0,0))
        prm = _lib.PrefilterParams.from_buffer_copy(params) if params is not None else _lib.default_prefilter()
        for i in range(3):
            prm.viewpoint[i] = float(np.float32(T[i, 3]))
        r = c.prefilter(cloud_in, prm, details=True)
        s, lab = r["sampled"], r["labels"]
        out = np.zeros((s.shape[0], 12), np.float32)
        out[:, :3] = s[:, :3]
        out[:, 3] = 1.0
        out[:, 4:7] = s[:, 4:7]
        out[:, 9] = s[:, 3]
        del clusters[:]
        order = np.argsort(lab, kind="stable")
        bounds = np.searchsorted(lab[order], np.arange(r["n_clusters"] + 1))
        for k in range(r["n_clusters"]):
            idx = order[bounds[k]:bounds[k + 1]]
            clusters.append(idx.astype(np.int32))
            out[idx, 8] = _cluster_rgb(k)
        return out
    kept = c.prefilter(cloud_in, params)
    if args and args[0] is not None:
        prev = np.asarray(args[0], np.float32).reshape(-1, 3)
        return np.concatenate([prev, kept], 0)
    return kept


def overlapFilter(cloudA, cloudB, poseA, poseB, range, angularView, accepted_pointsA=None, accepted_pointsB=None,
                  ctx=None):
    """filteringUtils.cpp:111-193 on the device (aicp_hip_fov_overlap): the FOV overlap in percent.
    cloudA / cloudB: (N, 3|4|8|12) float32 rows in the global frame; poseA / poseB: 4x4 poses.
    accepted_pointsA / accepted_pointsB: lists that receive the accepted points as one (M, 3)
    float32 array each (the reference appends to the clouds it is given)."""
    ov, ka, kb = _ctx(ctx).fov_overlap(cloudA, cloudB, poseA, poseB, range, angularView)
    if accepted_pointsA is not None:
        accepted_pointsA.append(ka)
    if accepted_pointsB is not None:
        accepted_pointsB.append(kb)
    return ov


def alignabilityFilter(cloudA, cloudB, poseA, poseB, cloudA_planes=None, cloudB_planes=None, eigenvectors=None,
                       ctx=None, params=None):
    """filteringUtils.cpp:196-430 on the device: the alignability in percent of two clouds that
    lie in the region of overlap (overlapFilter's accepted points): both are pre-filtered with the
    pose's translation as viewpoint, their plane clusters matched by box overlap and mean normal,
    and the matched normals analysed by PCA; 0 when no planes match. As the reference, it takes
    the accepted clouds from the host: aicp_hip_prefilter twice, then aicp_hip_cluster_match
    (Context.alignment_features is the call that chains the FOV filter, both pre-filters and the
    matching on the device). params: RiskParams (default_risk_params()).
    cloudA_planes / cloudB_planes / eigenvectors: lists that receive the matched planes ((M, 8)
    rows {x, y, z, nx, ny, nz, cluster, 0}) and the PCA frame ((3, 6) rows: the matched planes'
    centroid and one eigenvector each)."""
    c = _ctx(ctx)
    prm = params if params is not None else _lib.default_risk_params()
    pre = []
    for cloud, pose in ((cloudA, poseA), (cloudB, poseB)):
        pf = _lib.PrefilterParams.from_buffer_copy(prm.prefilter)
        T = np.asarray(pose, np.float64).reshape(4, 4)
        for i in range(3):
            pf.viewpoint[i] = float(np.float32(T[i, 3]))
        pre.append(c.prefilter(cloud, pf, details=True))
    (fa, fb) = pre
    r = c.cluster_match(fa["sampled"], fa["labels"], fb["sampled"], fb["labels"], prm.max_angle_deg,
                        tuple(prm.box_scale))
    for dst, f, ids in ((cloudA_planes, fa, [i for i in r["matching_indeces"] if i >= 0]),
                        (cloudB_planes, fb, [j for j, i in enumerate(r["matching_indeces"]) if i >= 0])):
        if dst is None:
            continue
        rows = [np.nonzero(f["labels"] == k)[0] for k in ids]
        idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        out = np.zeros((len(idx), 8), np.float32)
        out[:, :3] = f["sampled"][idx, :3]
        out[:, 3:6] = f["sampled"][idx, 4:7]
        out[:, 6] = f["labels"][idx]
        dst.append(out)
    if eigenvectors is not None and r["n_matches"]:
        eigenvectors.append(np.concatenate([np.tile(r["centroid"], (3, 1)), r["eigenvectors"].T], 1))
    return r["alignability"]
