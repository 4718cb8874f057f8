"""Independent checks of the CPU oracle (no GPU).

The oracle restates libpointmatcher/libnabo/octomap semantics that no in-repo golden vector
pins (parity unpinned). These tests check it against independent computations:
scipy cKDTree (exact kNN), numpy eigh (normals), numpy partition (quantile), numpy
solve/pinv (6x6 systems), a pure-Python DDA (octomap ray keys), Python's own text round trip
(ratio quantisation) and a numpy point-to-plane ICP restatement at epsilon = 0.
"""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

from aicp_mapping_amd import synthetic as sy
from overlap_reference import ray_keys as py_ray_keys


def rand_cloud(n, seed, scale=10.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-scale, scale, size=(n, 3))).astype(np.float32)


# ---------------------------------------------------------------- kd-tree ------------------
@pytest.mark.parametrize("k", [1, 4, 20])
def test_knn_eps0_matches_ckdtree(oracle, k):
    pts = rand_cloud(3000, 1)
    q = rand_cloud(500, 2)
    t = oracle.Tree(pts)
    ids, d2, tp, tn = t.knn(q, k=k, eps=0.0)
    dref, iref = cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=k)
    dref = np.asarray(dref).reshape(len(q), k) ** 2
    # ascending heap order, distances equal to float rounding
    assert np.all(np.diff(d2, axis=1) >= 0)
    np.testing.assert_allclose(d2, dref, rtol=2e-5, atol=1e-6)
    # the distances the oracle reports are the float distances of the ids it returns
    diff = q[:, None, :] - pts[ids]
    dd = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    np.testing.assert_array_equal(dd.astype(np.float32), d2)
    assert tp > 0 and tn > 0


def test_knn_self_match_allowed(oracle):
    pts = rand_cloud(1000, 3)
    ids, d2, _, _ = oracle.Tree(pts).knn(pts, k=1, eps=0.0)
    np.testing.assert_array_equal(ids[:, 0], np.arange(1000))
    assert np.all(d2 == 0)


@pytest.mark.parametrize("eps", [0.5, 3.16])
def test_knn_eps_bound(oracle, eps):
    pts = rand_cloud(5000, 4)
    q = rand_cloud(2000, 5)
    ids, d2, _, _ = oracle.Tree(pts).knn(q, k=1, eps=eps)
    dref, _ = cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=1)
    # libnabo guarantee: d <= (1 + eps) d_true  (squared here)
    assert np.all(d2[:, 0] <= (1 + eps) ** 2 * dref**2 * (1 + 1e-5) + 1e-6)
    assert np.any(d2[:, 0] > dref**2 * (1 + 1e-4))  # approximate search really is approximate


def test_knn_max_radius(oracle):
    pts = rand_cloud(2000, 6)
    q = rand_cloud(500, 7, scale=20)
    ids, d2, _, _ = oracle.Tree(pts).knn(q, k=1, eps=0.0, max_radius=0.5)
    dref, _ = cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=1)
    far = dref > 0.5 * (1 + 1e-5)
    assert np.all(ids[far, 0] == -1) and np.all(np.isinf(d2[far, 0]))
    near = dref < 0.5 * (1 - 1e-5)
    assert np.all(ids[near, 0] >= 0)


@pytest.mark.parametrize("seed", range(6))
def test_partition_prefix_form_equals_hoare(oracle, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 400))
    v = rng.integers(0, 12, size=n).astype(np.float32)  # many duplicates
    cut = np.float32(rng.integers(0, 12))
    a = oracle.partition(v, cut, parallel=False)
    b = oracle.partition(v, cut, parallel=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2:] == b[2:]
    assert np.all(a[0][: a[2]] < cut) and np.all(a[0][a[2] :] >= cut)
    assert np.all(a[0][a[2] : a[3]] == cut)


def test_tree_invariants(oracle):
    pts = rand_cloud(4000, 8)
    pts[:500] = pts[0]  # a block of duplicates
    t = oracle.Tree(pts)
    ex = t.export()
    n, depth, leaves = t.info()
    assert sorted(ex["bucket_ids"].tolist()) == list(range(4000))
    cd, cut, roc, bs = ex["cd"], ex["cut"], ex["right_or_count"], ex["bucket_start"]

    def ids_of(node):
        if cd[node] == 3:
            return ex["bucket_ids"][bs[node] : bs[node] + roc[node]].tolist()
        return ids_of(node + 1) + ids_of(roc[node])

    for node in range(n):
        if cd[node] == 3:
            assert 1 <= roc[node] <= 8
            continue
        L = pts[ids_of(node + 1), cd[node]]
        R = pts[ids_of(roc[node]), cd[node]]
        assert L.max() <= cut[node] <= R.min()
    assert leaves == int((cd == 3).sum()) and depth >= 9


# ---------------------------------------------------------------- normals ------------------
def test_normals_vs_eigh(oracle):
    P = sy.make_pair(6000, 10, seed=3).ref
    nrm, dens, deg = oracle.surface_normals(P, knn=20)
    assert deg == 0
    d, idx = cKDTree(P.astype(np.float64)).query(P.astype(np.float64), k=20)
    nb = P[idx].astype(np.float64)
    X = nb - nb.mean(1, keepdims=True)
    Cv = np.einsum("nki,nkj->nij", X, X) / 20
    w, V = np.linalg.eigh(Cv)
    ref = V[:, :, 0]
    gap = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-30)
    ok = gap > 1e-3
    dots = np.abs(np.sum(ref * nrm, 1))
    assert ok.mean() > 0.95
    assert np.all(dots[ok] > 1 - 1e-4)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
    # densities: k / (4/3 pi r_max^3)
    rmax = np.linalg.norm(X, axis=2).max(1)
    np.testing.assert_allclose(dens, 20 / (4.0 / 3.0 * math.pi * rmax**3), rtol=1e-4)


def test_normals_degenerate_line(oracle):
    x = np.linspace(0, 5, 200, dtype=np.float32)
    P = np.c_[x, np.zeros_like(x), np.zeros_like(x)].astype(np.float32)  # rank-1 neighbourhoods
    nrm, _, deg = oracle.surface_normals(P, knn=20)
    assert deg == 200
    np.testing.assert_array_equal(nrm, np.tile([0, 1, 0], (200, 1)).astype(np.float32))


# ---------------------------------------------------------------- quantile -----------------
@pytest.mark.parametrize("q", [0.25, 0.358818, 0.5, 0.7, 0.9999])
def test_quantile_vs_numpy(oracle, q):
    rng = np.random.default_rng(11)
    d2 = rng.exponential(size=10007).astype(np.float32)
    d2[::97] = np.inf
    d2[5:50] = d2[4]  # ties
    v, err = oracle.dists_quantile(d2, q)
    fin = d2[np.isfinite(d2)]
    k = int(np.float32(fin.size) * np.float32(q))
    assert err == 0 and v == np.partition(fin, k)[k]


def test_quantile_empty_and_max(oracle):
    v, err = oracle.dists_quantile(np.full(10, np.inf, np.float32), 0.5)
    assert err == 1
    d2 = np.arange(10, dtype=np.float32)
    assert oracle.dists_quantile(d2, 1.0) == (9.0, 0)


# ---------------------------------------------------------------- 6x6 solve ----------------
def test_solve6_full_rank(oracle):
    rng = np.random.default_rng(12)
    F = rng.normal(size=(6, 500))
    A = F @ F.T
    b = rng.normal(size=6)
    x, path = oracle.solve6(A, b)
    assert path == 0
    np.testing.assert_allclose(x, np.linalg.solve(A, b), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("rank", [1, 3, 5])
def test_solve6_rank_deficient_min_norm(oracle, rank):
    rng = np.random.default_rng(13 + rank)
    B = rng.normal(size=(6, rank))
    F = B @ rng.normal(size=(rank, 300))
    A = F @ F.T
    b = F @ rng.normal(size=300)  # in range(A), as b = -F dot in point-to-plane
    x, path = oracle.solve6(A, b)
    assert path in (1, 2)
    np.testing.assert_allclose(x, np.linalg.pinv(A) @ b, rtol=1e-6, atol=1e-9)


def test_solve6_planar_structure(oracle):
    # z = 0 clouds with normals e_z: F = [y, -x, 0, 0, 0, 1] -> rank 3
    rng = np.random.default_rng(14)
    p = rng.normal(size=(1000, 2))
    F = np.zeros((6, 1000))
    F[0], F[1], F[5] = p[:, 1], -p[:, 0], 1
    A = F @ F.T
    b = F @ rng.normal(size=1000)
    x, path = oracle.solve6(A, b)
    assert path == 1
    np.testing.assert_allclose(x, np.linalg.pinv(A) @ b, rtol=1e-8, atol=1e-12)
    assert x[2] == 0 and x[3] == 0 and x[4] == 0


# ---------------------------------------------------------------- octomap ray keys ---------
KMAX = 32768


def unpack(k):
    k = int(k)
    return ((k >> 32) & 0xFFFF, (k >> 16) & 0xFFFF, k & 0xFFFF)


RES = float(np.float32(0.2))  # YAMLConfigurator parses octomapResolution as<float>


@pytest.mark.parametrize("seed", range(4))
def test_ray_keys_vs_python(oracle, seed):
    rng = np.random.default_rng(seed)
    for _ in range(60):
        o = rng.uniform(-3, 3, 3).astype(np.float32)
        e = (o + rng.normal(0, 8, 3)).astype(np.float32)
        if seed == 3:  # axis-aligned and boundary cases
            e = o.copy()
            e[rng.integers(0, 3)] += np.float32(rng.integers(-20, 20) * 0.2)
        ks = oracle.ray_keys(o, e, RES)
        got = [unpack(k) for k in ks]
        assert got == py_ray_keys(o, e, RES)
        for a, b in zip(got, got[1:]):  # 6-connected traversal
            assert sum(abs(x - y) for x, y in zip(a, b)) == 1


def test_overlap_small_vs_python(oracle):
    pr = sy.make_pair(1500, 1500, seed=5, half=8.0)
    ov, cnt = oracle.overlap(pr.ref, pr.ref_origin, pr.read, pr.read_origin, RES)

    def keyset(P, org):
        S = set()
        o = np.asarray(org, np.float32)
        for p in P:
            S.update(py_ray_keys(o, p, RES))
            S.add(tuple(int(math.floor((1.0 / RES) * float(c))) + KMAX for c in p))
        return S

    A, B = keyset(pr.ref, pr.ref_origin), keyset(pr.read, pr.read_origin)
    assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (len(A), len(B), len(A & B))
    ta = np.float32(len(A & B)) / np.float32(len(A))
    tb = np.float32(len(A & B)) / np.float32(len(B))
    assert ov == np.float32(float(min(ta, tb)) * 100.0)


# ---------------------------------------------------------------- ratio auto-tune ----------
def test_quantize_ratio_text_round_trip(oracle):
    rng = np.random.default_rng(15)
    for r in np.concatenate([rng.uniform(0.25, 0.7, 2000), [0.25, 0.7, 0.358818]]).astype(np.float32):
        expect = np.float32(float("%g" % float(r)))
        assert oracle.quantize_ratio(r) == expect


@pytest.mark.parametrize("ov,expect", [(10.0, 0.25), (90.0, 0.7), (50.0, 0.5), (35.88183, 0.358818)])
def test_autotune_clamp(oracle, ov, expect):
    assert oracle.autotune_ratio(ov) == np.float32(expect)


# ---------------------------------------------------------------- whole ICP ----------------
def numpy_icp(ref, read, ratio, max_iter=20, min_rot=1e-3, min_trans=1e-2, smooth=4):
    """Independent numpy point-to-plane ICP with exact NN (epsilon 0) and eigh normals."""
    ref = ref.astype(np.float32)
    d, idx = cKDTree(ref.astype(np.float64)).query(ref.astype(np.float64), k=20)
    nb = ref[idx].astype(np.float64)
    X = nb - nb.mean(1, keepdims=True)
    w, V = np.linalg.eigh(np.einsum("nki,nkj->nij", X, X) / 20)
    nrm = V[:, :, 0].astype(np.float32)
    mu = (ref.astype(np.float64).sum(0) / len(ref)).astype(np.float32)
    refc = ref - mu
    readc = read.astype(np.float32) - mu
    tree = cKDTree(refc.astype(np.float64))
    T = np.eye(4, dtype=np.float32)
    hist = [np.eye(4)]
    it = 0
    while True:
        p = (readc @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        dd, ii = tree.query(p.astype(np.float64), k=1)
        diff = p - refc[ii]
        d2 = ((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]).astype(np.float32)
        k = int(np.float32(len(d2)) * np.float32(ratio))
        lim = np.partition(d2, k)[k]
        m = d2 <= lim
        pk, n = p[m].astype(np.float64), nrm[ii[m]].astype(np.float64)
        F = np.c_[np.cross(pk, n), n]
        dot = np.sum((pk - refc[ii[m]]) * n, 1)
        x = np.linalg.solve(F.T @ F, -(F.T @ dot))
        ang = np.linalg.norm(x[:3])
        ax = x[:3] / ang if ang > 0 else x[:3]
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dT = np.eye(4)
        dT[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
        dT[:3, 3] = x[3:]
        T = (dT.astype(np.float32) @ T).astype(np.float32)
        hist.append(T.astype(np.float64))
        it += 1
        if it >= max_iter:
            break
        if len(hist) > smooth:
            r = t = 0.0
            for i in range(len(hist) - 1, len(hist) - 1 - smooth, -1):
                r += sy.rot_err(hist[i - 1], hist[i])[0]
                t += np.linalg.norm(hist[i][:3, 3] - hist[i - 1][:3, 3])
            if r / smooth < min_rot and t / smooth < min_trans:
                break
    Tm = np.eye(4)
    Tm[:3, 3] = mu
    Ti = np.eye(4)
    Ti[:3, 3] = -mu
    return Tm @ T.astype(np.float64) @ Ti, it


def test_icp_eps0_vs_numpy_restatement(oracle):
    pr = sy.make_pair(6000, 6000, seed=2)
    cfg = oracle.default_config(nn_epsilon=0.0, trimmed_ratio=0.6)
    rc, T, st = oracle.icp(pr.ref, pr.read, cfg)
    assert rc == 0 and st.status == 0
    Tn, itn = numpy_icp(pr.ref, pr.read, 0.6)
    r, t = sy.rot_err(Tn, T)
    assert r < 2e-5 and t < 2e-4, (r, t)
    assert abs(st.iterations - itn) <= 1


def test_icp_recovers_ground_truth(oracle):
    pr = sy.make_pair(20000, 20000, seed=1)
    rc, T, st = oracle.icp(pr.ref, pr.read, oracle.default_config(trimmed_ratio=0.6))
    assert rc == 0
    r, t = sy.rot_err(pr.T_gt, T)
    assert r < 2e-3 and t < 2e-2
    assert st.converged == 1 and 4 <= st.iterations <= 20
    assert all(st.kept[i] == int(np.float32(20000) * np.float32(0.6)) + 1 or st.kept[i] >= 12000
               for i in range(st.iterations))


def test_icp_planar_scan_uses_min_norm_path(oracle):
    # 2-D scan lifted to z = 0: A has rank 3
    x = np.linspace(-5, 5, 400)
    P = np.c_[np.r_[x, x, np.full(400, -5.0)], np.r_[np.full(400, -3.0), np.full(400, 3.0), x * 0.6],
              np.zeros(1200)].astype(np.float32)
    T = sy.make_T(yaw_deg=1.0, pitch_deg=0, roll_deg=0, t=(0.05, 0.03, 0))
    R = sy.transform(np.linalg.inv(T), P)
    rc, Tout, st = oracle.icp(P, R, oracle.default_config(trimmed_ratio=0.7))
    assert rc == 0
    paths = [st.solve_path[i] for i in range(st.iterations)]
    assert 1 in paths or 2 in paths
    assert abs(Tout[2, 3]) < 1e-4  # unobservable z stays put (min-norm solution)


def test_c2_stall_is_the_epsilon_approximation(oracle):
    """The C2 stream's first pair (the first cloud vs reading 0, 120k points each; VERDICT r03
    item 2). With libnabo's approximate search (eps 3.16) the Differential checker stops ICP
    after ~10 iterations 0.025 rad / 0.13 m from the ground truth: the approximate matches
    move T by less than 1e-3 rad / 1e-2 m per step. Removing the approximation (eps 0)
    converges towards the ground truth in the oracle and in the independent numpy restatement
    alike, so the stall is the chain's behaviour, not a bug shared by oracle and device."""
    ref, o_ref = sy.stream_first(1, 120000)
    read, o_read, T_gt = sy.stream_reading(1, 0, 120000)
    ov, _ = oracle.overlap(ref, o_ref, read, o_read, float(np.float32(0.2)))
    ratio = oracle.autotune_ratio(ov)
    # eps 3.16 (the default chain): stops early, far from T_gt
    rc, T_eps, st_eps = oracle.icp(ref, read, oracle.default_config(trimmed_ratio=ratio))
    assert rc == 0 and st_eps.converged == 1 and st_eps.iterations < 20
    r, t = sy.rot_err(T_gt, T_eps)
    assert r > 0.01 and t > 0.05, (r, t)
    # eps 0: oracle and numpy agree and approach T_gt within the 20 iterations
    rc, T0, st0 = oracle.icp(ref, read, oracle.default_config(trimmed_ratio=ratio, nn_epsilon=0.0))
    assert rc == 0
    Tn, itn = numpy_icp(ref, read, ratio)
    r, t = sy.rot_err(Tn, T0)
    assert r < 2e-5 and t < 2e-4, (r, t)
    assert abs(st0.iterations - itn) <= 1
    for T in (T0, Tn):
        r, t = sy.rot_err(T_gt, T)
        assert r < 1e-3 and t < 1e-2, (r, t)
    # and eps 3.16 given more iterations (checker off) gets there too: slow, not wrong
    rc, T60, _ = oracle.icp(ref, read, oracle.default_config(trimmed_ratio=ratio, max_iter=60, min_diff_rot=1e-9,
                                                             min_diff_trans=1e-9))
    r, t = sy.rot_err(T_gt, T60)
    assert rc == 0 and r < 1e-3 and t < 2e-3, (r, t)


def test_c4_error_is_the_scene_not_the_chain(oracle):
    """C4's median 0.33 m from the ground truth (bench.py --config c4) on one
    of its crop pairs: bench.make_c4's reading 3 (120k points, drifted odometry) against the 1 M-
    point map cropped to +-15 m around its prior pose, r = 0.5 (app.cpp:41-51, 123-127). Unlike C2
    (test above) the approximation is not the cause: with eps 0 the oracle and the independent
    numpy ICP agree and stay ~0.2 m off too, and eps 3.16 run to 60 iterations with the checker
    off stays where the chain stopped (a fixed point, not a stall). The error lies along the
    direction of travel (x), the weakest direction of the point-to-plane translation information
    (sum of n n^T over the kept matches): the synthetic corridor has few surfaces facing x. So it
    is the scene's geometry, reproduced by every restatement, not a bug shared by oracle and device."""
    from scipy.spatial import cKDTree

    seed, i, n = 1, 3, 120000
    scene = sy.make_scene(seed)
    rng = np.random.default_rng(seed * 7919 + 77)
    mp = sy.sample_scene(scene, rng, np.array([0.0, 0.0, 0.7]), half=40.0)
    mp = mp[rng.choice(len(mp), size=1000000, replace=False)].astype(np.float32)
    read, _, Tg = sy.stream_reading(seed, i, n)
    pose = np.linalg.inv(Tg) @ sy.make_T(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0, t=((i + 1) * 0.3, 0.0, 0.7))
    crop, _ = oracle.crop_box(mp, -15.0, 15.0, pose)
    assert 150000 < len(crop) < 200000
    rc, T, st = oracle.icp(crop, read, oracle.default_config(trimmed_ratio=0.5))
    assert rc == 0 and st.converged == 1
    r, t = sy.rot_err(Tg, T)
    assert t > 0.3, (r, t)
    # eps 0: oracle == numpy, and still off
    rc, T0, _ = oracle.icp(crop, read, oracle.default_config(trimmed_ratio=0.5, nn_epsilon=0.0))
    Tn, _ = numpy_icp(crop, read, 0.5)
    r0, t0 = sy.rot_err(Tn, T0)
    assert rc == 0 and r0 < 2e-5 and t0 < 2e-4, (r0, t0)
    assert sy.rot_err(Tg, T0)[1] > 0.1
    # eps 3.16 with 60 iterations and no differential stop: the same place
    rc, T60, _ = oracle.icp(crop, read, oracle.default_config(trimmed_ratio=0.5, max_iter=60, min_diff_rot=1e-9,
                                                              min_diff_trans=1e-9))
    r6, t6 = sy.rot_err(T60, T)
    assert rc == 0 and r6 < 1e-3 and t6 < 1e-3, (r6, t6)
    # the error is along the weakest direction of the translation information
    tree = cKDTree(crop.astype(np.float64))
    _, idx = tree.query(crop.astype(np.float64), k=20)
    nb = crop[idx].astype(np.float64)
    X = nb - nb.mean(1, keepdims=True)
    nrm = np.linalg.eigh(np.einsum("nki,nkj->nij", X, X))[1][:, :, 0]
    moved = read.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]
    dd, j = tree.query(moved)
    N = nrm[j[dd <= np.quantile(dd, 0.5)]]
    ew, ev = np.linalg.eigh(N.T @ N / len(N))
    err = T[:3, 3].astype(np.float64) - Tg[:3, 3]
    assert ew[0] < 0.05 * ew[2], ew
    assert abs(ev[:, 0] @ err) > 0.99 * np.linalg.norm(err), (ev[:, 0], err)
    assert abs(ev[0, 0]) > 0.99  # that direction is x, the direction of travel


def test_sequence_debug_mode_replay(oracle):
    """The oracle's replay of App's debug working mode (app.cpp:87-96, 414) on a short stream:
    reading 0 sees initialT_ = identity (so it equals robot mode's first registration); every
    later reading is registered as initialT_ * reading with prior origin initialT_ * prior pose,
    initialT_ being the float product of the accepted corrections so far; a dropped reading
    leaves it unchanged."""
    st = sy.make_stream(n_readings=6, n_points=3000, seed=5, half=12.0, jumps={3: (0.6, 0, 0)})
    dbg = oracle.sequence(st.first, st.first_origin, st.readings, st.origins, max_correction_magnitude=0.4,
                          resolution=RES, working_mode="debug")
    rob = oracle.sequence(st.first, st.first_origin, st.readings[:1], st.origins[:1], max_correction_magnitude=0.4,
                          resolution=RES)
    np.testing.assert_array_equal(dbg[0]["T"], rob[0]["T"])
    assert [r["accepted"] for r in dbg] == [1, 1, 1, 0, 1, 1]
    initT = np.eye(4, dtype=np.float32)
    for i, r in enumerate(dbg):
        np.testing.assert_allclose(r["prior_origin"], oracle.corrected_origin(initT, st.origins[i]), rtol=0, atol=0)
        if r["accepted"]:
            initT = oracle.mul4(r["T"], initT)
    # the drift is absorbed after the first correction: later accepted corrections are small
    for r in dbg[1:]:
        if r["accepted"]:
            assert sy.rot_err(np.eye(4), r["T"])[0] < 5e-3
