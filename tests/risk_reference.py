"""numpy restatement of the alignment-risk features, the reference side of test_alignment_risk.py
(used by tests only): overlapFilter (aicp_core/src/utils/filteringUtils.cpp:111-193) with the
device's expressions (double, then float32), and boxes, counts, matching and PCA of
alignabilityFilter (:196-430, helpers :432-576) in double. tests/test_risk_reference.py checks it
against independent computations."""
import numpy as np

F32 = np.float32


def pose(yaw_deg=0.0, t=(0.0, 0.0, 0.0)):
    """4x4 row-major pose: a yaw and a translation."""
    a = np.deg2rad(yaw_deg)
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    P[:3, 3] = t
    return P


def pose_inverse(P):
    """R^T and -R^T t in double with explicit left-to-right sums (3 x 4)."""
    P = np.asarray(P, np.float64)
    R, t = P[:3, :3], P[:3, 3]
    inv = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            inv[r, c] = R[c, r]
        inv[r, 3] = -((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2])
    return inv


def fov_filter(cloud, other_pose, range_m, angular_view, r_band=1e-4):
    """One half of overlapFilter: dict(kept = accepted points (float32, global frame, input
    order), mask, borderline = number of points within 1e-4 deg of the angle bound or r_band
    metres of the range)."""
    P = np.asarray(other_pose, np.float64)
    xyz = np.asarray(cloud, F32)[:, :3].astype(np.float64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    inv = pose_inverse(P)
    q = np.empty((len(xyz), 3), F32)
    for r in range(3):
        q[:, r] = (((inv[r, 0] * x + inv[r, 1] * y) + inv[r, 2] * z) + inv[r, 3]).astype(F32)
    qd = q.astype(np.float64)
    rad = np.sqrt((qd[:, 0] * qd[:, 0] + qd[:, 1] * qd[:, 1]) + qd[:, 2] * qd[:, 2])
    theta = np.arctan2(qd[:, 1], qd[:, 0]) * 180.0 / np.pi
    thresh = float(F32(180.0 - ((360.0 - float(F32(angular_view))) / 2)))
    rng = float(F32(range_m))
    mask = (theta < thresh) & (theta > -thresh) & (rad < rng)
    Rf, tf = P[:3, :3].astype(F32), P[:3, 3].astype(F32)
    g = np.empty_like(q)
    for r in range(3):
        g[:, r] = ((Rf[r, 0] * q[:, 0] + Rf[r, 1] * q[:, 1]) + Rf[r, 2] * q[:, 2]) + tf[r]
    assert g.dtype == F32
    borderline = int(((np.abs(np.abs(theta) - thresh) < 1e-4) | (np.abs(rad - rng) < r_band)).sum())
    return dict(kept=g[mask], mask=mask, borderline=borderline)


def fov_overlap_value(kept_a, n_a, kept_b, n_b):
    pa = F32(kept_a) / F32(n_a)
    pb = F32(kept_b) / F32(n_b)
    return F32(np.float64(F32(pa * pb)) * 100.0)


def clusters_of(sampled, labels):
    """Index lists of clusters 0 .. max label, each in sampled-cloud order."""
    labels = np.asarray(labels)
    nc = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0
    return [np.nonzero(labels == c)[0] for c in range(nc)]


def _fix_sign(v):
    """The axis with its component of largest magnitude (the first of equals) positive."""
    return -v if v[np.argmax(np.abs(v))] < 0 else v


def crop_frame(rot):
    """The rotation pcl::CropBox builds from getPointsInOrientedBox's angles (:484-499), in double:
    Eigen's eulerAngles(0, 1, 2) of rot, for which rot = Rx(a) Ry(b) Rz(c), handed to
    pcl::getTransformation, which composes Rz(c) Ry(b) Rx(a). The two agree for a rotation about one
    axis only; the box the reference counts in is this one."""
    R = np.asarray(rot, np.float64)
    a0 = np.arctan2(R[1, 2], R[2, 2])
    c2 = np.sqrt(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1])
    if a0 > 0:
        a0 -= np.pi
        a1 = np.arctan2(-R[0, 2], -c2)
    else:
        a1 = np.arctan2(-R[0, 2], c2)
    s1, c1 = np.sin(a0), np.cos(a0)
    a2 = np.arctan2(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    rx, ry, rz = -a0, -a1, -a2
    A, B, C, D, E, F = np.cos(rz), np.sin(rz), np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    return np.array([[A * C, A * D * F - B * E, B * F + A * D * E], [B * C, A * E + B * D * F, B * D * E - A * F],
                     [-D, C * F, C * E]])


def cluster_box(points, scale=(1.0, 1.0, 3.0)):
    """MomentOfInertiaEstimation::getOBB of a cluster after overlapBoxFilter's scaling, in double:
    dict(centre, rot (columns major, middle = minor x major, minor; one fixed sign per axis), half,
    frame = crop_frame(rot), the rotation the points are counted in)."""
    P = np.asarray(points, np.float64)
    mean = P.mean(0)
    D = P - mean
    w, V = np.linalg.eigh(D.T @ D / len(P))
    major, minor = _fix_sign(V[:, 2]), _fix_sign(V[:, 0])
    rot = np.stack([major, np.cross(minor, major), minor], 1)
    L = D @ rot
    lo, hi = L.min(0), L.max(0)
    return dict(centre=mean + rot @ ((hi + lo) / 2), rot=rot, half=(hi - lo) / 2 * np.asarray(scale, np.float64),
                frame=crop_frame(rot))


def box_counts(boxes, sampled, labels, n_clusters):
    """Points of every cluster of a cloud in every box of the other, as bounds: (inner, outer)
    integer arrays [box][cluster]: strictly inside the box shrunk by delta = 1e-4 half + 1e-5 m, and
    inside the box grown by delta, in CropBox's frame of the box."""
    P = np.asarray(sampled, np.float64)[:, :3]
    labels = np.asarray(labels)
    inner = np.zeros((len(boxes), n_clusters), np.int64)
    outer = np.zeros_like(inner)
    sel = labels >= 0
    for b, bx in enumerate(boxes):
        L = np.abs((P[sel] - bx["centre"]) @ bx["frame"])
        d = 1e-4 * bx["half"] + 1e-5
        inner[b] = np.bincount(labels[sel][(L < bx["half"] - d).all(1)], minlength=n_clusters)
        outer[b] = np.bincount(labels[sel][(L <= bx["half"] + d).all(1)], minlength=n_clusters)
    return inner, outer


def overlap_table(a_in_b, b_in_a, size_a, size_b):
    """overlapBoxFilter's value (:565-575) for every pair, float32 [clusters_A][clusters_B];
    a_in_b: [B][A], b_in_a: [A][B]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        pa = np.asarray(a_in_b).T.astype(F32) / np.asarray(size_a, F32)[:, None]
        pb = np.asarray(b_in_a).astype(F32) / np.asarray(size_b, F32)[None, :]
        return ((pa * pb).astype(np.float64) * 100.0).astype(F32)


def angle_table(sum_n_a, size_a, sum_n_b, size_b):
    """Angle in degrees (float32) between the clusters' mean normals, the cosine clamped to
    [-1, 1]; NaN with a zero-length mean."""
    ca = np.asarray(sum_n_a, np.float64) / np.asarray(size_a, np.float64)[:, None]
    cb = np.asarray(sum_n_b, np.float64) / np.asarray(size_b, np.float64)[:, None]
    den = np.linalg.norm(ca, axis=1)[:, None] * np.linalg.norm(cb, axis=1)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.clip((ca @ cb.T) / den, -1.0, 1.0)
        ang = np.arccos(c) * 180.0 / np.pi
    ang[~(den > 0)] = np.nan
    return ang.astype(F32)


def match(overlap, angle, max_angle=20.0):
    """filteringUtils.cpp:236-286 by tables: every A-cluster takes the B-cluster of largest overlap
    among those closer than max_angle (first on ties, overlap > 0); every B-cluster keeps the
    claimant of largest overlap (first on ties). Returns (matching_indeces, matching_overlap,
    matching_distance)."""
    na, nb = overlap.shape
    ok = (angle < F32(max_angle)) & (overlap > 0)
    ov = np.where(ok, overlap, F32(-1))
    idx = np.full(nb, -1, np.int32)
    mo = np.full(nb, -1, F32)
    md = np.full(nb, -1, F32)
    if na == 0 or nb == 0:
        return idx, mo, md
    best = ov.argmax(1)                       # first maximum
    has = ov[np.arange(na), best] > 0
    for j in range(nb):
        cl = np.nonzero(has & (best == j))[0]
        if cl.size:
            i = cl[overlap[cl, j].argmax()]   # first maximum among the claimants
            idx[j], mo[j], md[j] = i, overlap[i, j], angle[i, j]
    return idx, mo, md


def pca(sum_nn_a, matching_indeces):
    """PCA of the matched A-clusters' normals and their mirror images (:288-400): the centroid is
    exactly zero, the matrix the sum of the clusters' sum n n^T. sum_nn_a: [cluster] 3 x 3.
    Returns (alignability float32, normalised eigenvalues descending, eigenvectors as columns)."""
    sel = [i for i in matching_indeces if i >= 0]
    if not sel:
        return F32(0), np.zeros(3), np.zeros((3, 3))
    S = np.zeros((3, 3))
    for i in sel:
        S = S + sum_nn_a[i]
    w, V = np.linalg.eigh(S)
    w, V = w[::-1], V[:, ::-1]
    return F32(100.0 * (w[2] / w[0])) if w[0] > 0 else F32(0), w / w.sum(), V


def cluster_sums(sampled, labels):
    """Per cluster: size, points (double), sum n, sum n n^T."""
    S = np.asarray(sampled, np.float64)
    out = []
    for idx in clusters_of(sampled, labels):
        N = S[idx, 4:7]
        out.append(dict(size=len(idx), points=S[idx, :3], sum_n=N.sum(0), sum_nn=N.T @ N))
    return out


def alignability(sampled_a, labels_a, sampled_b, labels_b, max_angle=20.0, scale=(1.0, 1.0, 3.0), counts=None):
    """alignabilityFilter after its two pre-filters. counts: (a_in_b, b_in_a) to match with (the
    device's, once they are known to lie within the bounds); default: the inner bounds. Returns a
    dict with boxes, count bounds, tables, matching arrays, alignability, eigenvalues, eigenvectors,
    centroid and `stable` (the inner and the outer counts give the same matching_indeces)."""
    A, B = cluster_sums(sampled_a, labels_a), cluster_sums(sampled_b, labels_b)
    na, nb = len(A), len(B)
    empty = np.zeros(0, np.int64)
    boxes_a = [cluster_box(c["points"], scale) if c["size"] else None for c in A]
    boxes_b = [cluster_box(c["points"], scale) if c["size"] else None for c in B]
    assert all(b is not None for b in boxes_a + boxes_b), "every label up to the largest must be used"
    ab_in, ab_out = box_counts(boxes_b, sampled_a, labels_a, na)   # [B][A]
    ba_in, ba_out = box_counts(boxes_a, sampled_b, labels_b, nb)   # [A][B]
    size_a = np.array([c["size"] for c in A] or empty)
    size_b = np.array([c["size"] for c in B] or empty)
    ang = angle_table(np.array([c["sum_n"] for c in A]).reshape(na, 3), size_a,
                      np.array([c["sum_n"] for c in B]).reshape(nb, 3), size_b) if na and nb else np.zeros((na, nb), F32)
    res = {}
    for name, (ab, ba) in dict(inner=(ab_in, ba_in), outer=(ab_out, ba_out),
                               used=counts if counts is not None else (ab_in, ba_in)).items():
        ov = overlap_table(ab, ba, size_a, size_b) if na and nb else np.zeros((na, nb), F32)
        res[name] = (ov,) + match(ov, ang, max_angle)
    ov, idx, mo, md = res["used"]
    al, ev, evec = pca([c["sum_nn"] for c in A], idx)
    sel = [i for i in idx if i >= 0]
    cen = (np.concatenate([A[i]["points"] for i in sel]).mean(0) if sel else np.zeros(3))
    return dict(boxes_a=boxes_a, boxes_b=boxes_b, a_in_b=(ab_in, ab_out), b_in_a=(ba_in, ba_out), size_a=size_a,
                size_b=size_b, overlap=ov, angle=ang, matching_indeces=idx, matching_overlap=mo, matching_distance=md,
                alignability=al, eigenvalues=ev, eigenvectors=evec, centroid=cen, n_matches=len(sel),
                stable=bool(np.array_equal(res["inner"][1], res["outer"][1])))
