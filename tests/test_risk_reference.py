"""The numpy restatement of the alignment-risk features (tests/risk_reference.py) against
independent computations: it is the reference side of test_alignment_risk.py."""
import numpy as np

import risk_reference as rr


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_box_of_a_rotated_cuboid():
    """A filled 2 x 1 x 0.2 lattice, rotated and moved: the box has the lattice's frame (axes up to
    sign, major / middle / minor by extent), centre and half extents, the minor one scaled by 3."""
    g = np.stack(np.meshgrid(np.linspace(-1, 1, 21), np.linspace(-0.5, 0.5, 11), np.linspace(-0.1, 0.1, 5),
                             indexing="ij"), -1).reshape(-1, 3)
    R, t = _rot(0.3, -0.7, 1.1), np.array([4.0, -2.0, 0.5])
    b = rr.cluster_box(g @ R.T + t)
    np.testing.assert_allclose(b["centre"], t, atol=1e-12)
    np.testing.assert_allclose(b["half"], [1.0, 0.5, 0.3], atol=1e-12)
    np.testing.assert_allclose(np.abs(np.sum(b["rot"] * R, 0)), 1.0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(b["rot"]), 1.0, atol=1e-12)
    np.testing.assert_allclose(np.cross(b["rot"][:, 2], b["rot"][:, 0]), b["rot"][:, 1], atol=1e-12)


def test_box_is_symmetric_for_a_lopsided_cluster():
    """getOBB shifts the centre to the middle of the extents: every point lies inside, and each
    face is touched."""
    rng = np.random.default_rng(5)
    P = rng.random((500, 3)) ** 2 * [3.0, 1.0, 0.05] + [1.0, 2.0, 3.0]
    b = rr.cluster_box(P, scale=(1, 1, 1))
    L = (P - b["centre"]) @ b["rot"]
    np.testing.assert_allclose(L.max(0), b["half"], atol=1e-12)
    np.testing.assert_allclose(L.min(0), -b["half"], atol=1e-12)


def test_counts_of_a_lattice_in_a_known_box():
    """An axis-aligned box of half extents (1, 0.5, 0.1 x 3) around the origin and a 0.25 m
    lattice labelled by the sign of x: the counts are the lattice points inside, none borderline."""
    box = dict(centre=np.zeros(3), frame=np.eye(3), half=np.array([1.0, 0.5, 0.3]))
    ax = np.arange(-2.0, 2.0001, 0.25) + 0.1
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    lab = (g[:, 0] > 0).astype(np.int32)
    lab[::7] = -1
    s = np.zeros((len(g), 8), np.float32)
    s[:, :3] = g
    inner, outer = rr.box_counts([box], s, lab, 2)
    inside = (np.abs(g[:, 0]) <= 1.0) & (np.abs(g[:, 1]) <= 0.5) & (np.abs(g[:, 2]) <= 0.3) & (lab >= 0)
    want = [int((inside & (lab == 0)).sum()), int((inside & (lab == 1)).sum())]
    assert want[0] > 0 and want[1] > 0
    assert inner.tolist() == [want] and outer.tolist() == [want]


def test_crop_frame_is_the_rotation_for_one_axis_and_pcl_s_order_otherwise():
    """rot = Rx(a) Ry(b) Rz(c) gives Rz(c) Ry(b) Rx(a): equal for a rotation about one axis."""
    for R in (_rot(0.4, 0, 0), _rot(0, -1.2, 0), _rot(0, 0, 2.5), np.eye(3)):
        np.testing.assert_allclose(rr.crop_frame(R), R, atol=1e-12)
    a, b, c = 0.3, -0.7, 1.1
    Rx, Ry, Rz = _rot(a, 0, 0), _rot(0, b, 0), _rot(0, 0, c)
    np.testing.assert_allclose(rr.crop_frame(Rx @ Ry @ Rz), Rz @ Ry @ Rx, atol=1e-12)
    assert np.abs(Rx @ Ry @ Rz - Rz @ Ry @ Rx).max() > 0.1


def test_pca_of_analytic_normal_sets():
    e = np.eye(3)
    nn = [np.outer(v, v) * 10 for v in e]
    al, ev, _ = rr.pca(nn, [0, 1, 2])
    assert al == np.float32(100) and np.allclose(ev, 1 / 3)
    al, ev, vec = rr.pca(nn, [2, -1, -1])
    assert al == 0 and np.allclose(ev, [1, 0, 0]) and np.allclose(np.abs(vec[:, 0]), [0, 0, 1])
    al, ev, _ = rr.pca([nn[0] * 4, nn[1] * 2, nn[2]], [0, 1, 2])   # 40 : 20 : 10
    assert al == np.float32(25.0) and np.allclose(ev, [4 / 7, 2 / 7, 1 / 7])
    assert rr.pca(nn, [-1, -1])[0] == 0


def _sequential(overlap, angle, max_angle=20.0):
    """filteringUtils.cpp:226-286, line by line."""
    na, nb = overlap.shape
    idx, mo, md = [-1] * nb, [-1.0] * nb, [-1.0] * nb
    for i in range(na):
        max_overlap, current_distance, k = 0.0, -1.0, -1
        for j in range(nb):
            if overlap[i, j] > max_overlap and angle[i, j] < max_angle:
                k, max_overlap, current_distance = j, overlap[i, j], angle[i, j]
        if max_overlap > 0:
            if idx[k] == -1 or max_overlap > mo[k]:
                idx[k], mo[k], md[k] = i, max_overlap, current_distance
    return idx, mo, md


def test_matching_against_the_sequential_logic():
    rng = np.random.default_rng(11)
    for trial in range(200):
        na, nb = rng.integers(0, 9, 2)
        ov = rng.integers(0, 4, (na, nb)).astype(np.float32) * np.float32(12.5)   # many ties and zeros
        ang = rng.choice(np.array([0.0, 5.0, 19.0, 21.0, 90.0, np.nan], np.float32), (na, nb))
        idx, mo, md = rr.match(ov, ang)
        sidx, smo, smd = _sequential(ov, ang)
        assert idx.tolist() == sidx, (trial, ov, ang)
        assert mo.tolist() == smo and md.tolist() == smd


def test_fov_restatement_against_a_direct_computation():
    """The float32 / double expressions against plain double geometry, away from the bounds."""
    rng = np.random.default_rng(2)
    P = (rng.random((4000, 3)) * 8 - 4).astype(np.float32)
    other = rr.pose(30.0, (0.6, 0.3, 0.7))
    r = rr.fov_filter(P, other, 5.0, 270.0)
    q = (P.astype(np.float64) - other[:3, 3]) @ other[:3, :3]
    th = np.degrees(np.arctan2(q[:, 1], q[:, 0]))
    far = (np.abs(np.abs(th) - 135.0) > 1e-3) & (np.abs(np.linalg.norm(q, axis=1) - 5.0) > 1e-3)
    want = (np.abs(th) < 135.0) & (np.linalg.norm(q, axis=1) < 5.0)
    assert np.array_equal(r["mask"][far], want[far]) and 0 < want.sum() < len(P)
    np.testing.assert_allclose(r["kept"], P[r["mask"]], atol=2e-6)   # there and back in float
    assert rr.fov_overlap_value(1, 2, 1, 2) == np.float32(25.0)
