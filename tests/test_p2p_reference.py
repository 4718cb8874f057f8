"""The reference of test_p2p_step_kernels.py, pinned on the CPU independently of the device: its
3x3 SVD rotation against numpy.linalg.svd's Kabsch solution in double, exact correspondences, the
reflection and rank rules, the comparison's sharpness (MUTATIONS) and the margins of every input the
GPU tests run. Plus the argument checks of aicp_hip_test_step_p2p, which come before any device work.

Measured (the GPU cases' M and 2000 random ones, graded down to sig_2 / sig_0 = 1e-6): max |R - R_np|
3.8e-12 where sig_1 / sig_0 >= 1e-3 (bar 2^-30 = 9.3e-10); no case misses the bar. The objective is
taken as tr(R^T M) = sum_ab R_ab M_ab with M = sum q p^T: that is the quantity R = U V^T maximises
(tr(R M) without the transpose is not an objective of this M).
"""
import ctypes as C
import math

import numpy as np
import pytest

import p2p_reference as pr
import step_reference as sr

f32, f64 = np.float32, np.float64
BAR = 2.0 ** -30   # 1/64 of a float ulp at 1: dT is rounded to float32


def kabsch_np(M):
    """The proper rotation maximising tr(R^T M), by numpy's SVD in double."""
    Un, sn, Vtn = np.linalg.svd(np.asarray(M, f64))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Un @ Vtn) >= 0 else -1.0])
    return Un @ D @ Vtn, sn


def case_Ms():
    """(name, M) of every update the GPU cases make, from the reference's own simulation."""
    out = []
    for name in sorted(pr.CASES):
        if name in ("rows129",) or name.startswith("ring") and name != "ring4":
            continue   # (same kind of M as the others; kept out for time)
        case = pr.get_case(name)
        got = pr.simulate(case)
        _, _, nrow, roff = sr.layout(case)
        S, P = got["kept"].shape
        act = [bool(st.active) for st in sr.initial_states(case)]
        for s in range(S):
            for p in range(P):
                rows = got["slab"][s, roff[p]:roff[p + 1]]
                if act[p] and got["kept"][s, p] > 0:
                    tot = pr.total_from_rows(rows)
                    out.append((f"{name}/{s}/{p}", np.array(pr.cross_covariance(tot)[2], f64)))
                act[p] = bool(got["active"][s, p])
    return out


def random_Ms(n=2000):
    rng = np.random.default_rng(3)
    out = []
    for i in range(n):
        M = rng.normal(size=(3, 3))
        kind = i % 5
        if kind == 1:     # graded singular values down to 1e-6
            u, _, vt = np.linalg.svd(M)
            M = u @ np.diag([1.0, 10.0 ** rng.uniform(-3, 0), 10.0 ** rng.uniform(-6, 0)]) @ vt
        elif kind == 2:   # exact rank 2
            M[:, 2] = M[:, 0] - 2 * M[:, 1]
        elif kind == 3:   # scaled
            M *= 10.0 ** rng.uniform(-8, 12)
        elif kind == 4:   # a reflection times a well-conditioned spd matrix
            u, _, vt = np.linalg.svd(M)
            M = u @ np.diag([3.0, 2.0, 1.0]) @ vt
            if np.linalg.det(M) > 0:
                M = -M
        out.append((f"random{i}", M))
    return out


def check_rotation(name, M, worst):
    R, rank = pr.p2p_rotation(M)
    R = np.array(R, f64)
    Rn, sn = kabsch_np(M)
    s0 = sn[0]
    if rank >= 2:
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, name
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12, name
        assert np.sum(R * M) >= np.sum(Rn * M) - 1e-12 * s0, name
    else:
        assert np.array_equal(R, np.eye(3)), name
    if s0 > 0 and sn[1] / s0 >= 1e-3 and rank >= 2:
        d = np.abs(R - Rn).max()
        worst[0] = max(worst[0], d)
        assert d <= BAR, (name, d)


def test_svd_rotation_against_numpy_kabsch(oracle):
    worst = [0.0]
    Ms = case_Ms()
    assert len(Ms) > 100
    for name, M in Ms + random_Ms():
        check_rotation(name, M, worst)
    print(f"max |R - R_np| where sig_1 / sig_0 >= 1e-3: {worst[0]:.3e} (bar {BAR:.3e})")


def test_svd3_factors():
    """U diag(sig) V^T = M, orthonormal V, sig descending (ties by index: a stable order)."""
    for name, M in random_Ms(300):
        Um, sig, V = pr.svd3(M)
        Um, sig, V = np.array(Um), np.array(sig), np.array(V)
        assert sig[0] >= sig[1] >= sig[2] >= 0, name
        scale = max(sig[0], 1e-300)
        assert np.abs(Um @ np.diag(sig) @ V.T - M).max() <= 1e-14 * scale, name
        assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-14, name
    Um, sig, V = pr.svd3(np.diag([2.0, 2.0, 2.0]))
    assert [float(v) for v in sig] == [2.0, 2.0, 2.0] and np.array_equal(np.array(V), np.eye(3))
    Um, sig, V = pr.svd3(np.diag([1.0, 3.0, 3.0]))   # ties keep their index order: columns 1, 2, then 0
    assert [float(v) for v in sig] == [3.0, 3.0, 1.0]
    assert np.array_equal(np.array(V), np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]))


def test_exact_correspondences_return_the_transform():
    """A subset of the reference moved by a known rigid transform, ratio 1: one step returns it
    within the parity bar, 1e-6 rad / 1e-5 m."""
    from aicp_mapping_amd import synthetic as sy

    case = pr.get_case("exact")
    got = pr.simulate(case)
    assert got["kept"][0, 0] == case["n_read"][0] == 300
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = pr.EXACT_R, pr.EXACT_T
    # the solution in double, by the project's measure (acos of the trace)
    tot = pr.total_from_rows(got["slab"][0])
    pm, qm, M = pr.cross_covariance(tot)
    R = np.array(pr.p2p_rotation(M)[0], f64)
    Td = np.eye(4)
    Td[:3, :3], Td[:3, 3] = R, np.array(qm, f64) - R @ np.array(pm, f64)
    r, t = sy.rot_err(want, Td)
    print(f"exact correspondences, double: {r:.2e} rad, {t:.2e} m")
    assert r <= 1e-6 and t <= 1e-5, (r, t)
    # T_iter, rounded to float32. acos((tr - 1) / 2) of a matrix whose entries carry 3e-8 of rounding
    # cannot resolve angles below sqrt(2 * 1e-7) = 4e-4 rad, so the angle is taken from the
    # antisymmetric part, sin(angle) = |vee(D - D^T)| / 2, which is accurate at 0
    T = got["T"][0, 0].reshape(4, 4).T.astype(f64)
    D = np.linalg.inv(want) @ T
    A = D[:3, :3] - D[:3, :3].T
    r = math.asin(min(1.0, 0.5 * math.sqrt(A[2, 1] ** 2 + A[0, 2] ** 2 + A[1, 0] ** 2)))
    t = float(np.linalg.norm(D[:3, 3]))
    print(f"exact correspondences, T_iter in float32: {r:.2e} rad, {t:.2e} m")
    assert r <= 1e-6 and t <= 1e-5, (r, t)


def test_reflection_case_yields_a_proper_rotation():
    case = pr.get_case("reflection")
    got = pr.simulate(case)
    _, _, _, roff = sr.layout(case)
    M = np.array(pr.cross_covariance(pr.total_from_rows(got["slab"][0, roff[0]:roff[1]]))[2])
    Un, sn, Vtn = np.linalg.svd(M)
    assert np.linalg.det(Un @ Vtn) < 0 and sn[2] / sn[0] > 1e-5      # the unconstrained optimum reflects
    R, rank = pr.p2p_rotation(M)
    assert rank == 3 and abs(np.linalg.det(np.array(R, f64)) - 1.0) <= 1e-12
    Rbad, _ = pr.p2p_rotation(M, "no_det_fix")
    assert np.linalg.det(np.array(Rbad, f64)) < -0.99
    T = got["T"][0, 0].reshape(4, 4).T
    assert np.linalg.det(T[:3, :3].astype(f64)) > 0.999 and got["status"][0, 0] == 0


def test_rank_rule():
    """Rank-1 and one-point cases take R = I with t = qm - pm; the ranks case reaches 3, 2, 1, 0; a
    family of M sits across the 3 FLT_EPSILON threshold on both sides."""
    case = pr.get_case("ranks")
    got = pr.simulate(case)
    info = pr.compare(case, got)
    assert tuple(info["ranks"][0]) == pr.RANKS
    assert got["kept"][0, 3] == 1
    _, _, _, roff = sr.layout(case)
    for p in (2, 3):
        tot = pr.total_from_rows(got["slab"][0, roff[p]:roff[p + 1]])
        dT, rank = pr.delta_from_totals(tot)
        assert rank < 2 and np.array_equal(dT.reshape(4, 4).T[:3, :3], np.eye(3, dtype=f32))
        n = tot[27]
        assert np.array_equal(dT[12:15], ((tot[12:15] / n) - (tot[9:12] / n)).astype(f32))
    # the threshold itself, on diagonal M: sig_1 or sig_2 on either side of sig_0 * 3 FLT_EPSILON
    thr = 3.0 * pr.FLT_EPS
    for k, want in ((np.nextafter(thr, 1), 3), (thr, 2), (thr / 2, 2)):
        assert pr.p2p_rotation(np.diag([1.0, 0.5, k]))[1] == want
    for k, want in ((np.nextafter(thr, 1), 2), (thr, 1)):
        assert pr.p2p_rotation(np.diag([1.0, k, 0.0]))[1] == want
    assert pr.p2p_rotation(np.zeros((3, 3)))[1] == 0
    t = pr.compare(pr.get_case("threshold"), pr.simulate(pr.get_case("threshold")))["ranks"][0]
    assert t[0] == 2 and t[-1] == 3 and t == sorted(t), t
    k = t.index(3)
    assert 3 <= k <= 12, t   # the rank changes inside the fine steps around the threshold


# ------------------------------------------------------------------ the comparison is sharp
MUTANT_CASE = dict(lt=("ties",), drop_tail=("tail1025",), ref_off=("ragged",), transposeM=("exact", "ranks"),
                   no_det_fix=("reflection",), no_means=("exact", "ranks"), rows128=("rows129",))


def test_every_mutation_has_a_case():
    assert set(MUTANT_CASE) == set(pr.MUTATIONS)
    assert {"lt", "drop_tail", "ref_off", "transposeM", "no_det_fix", "no_means"} <= set(pr.MUTATIONS)


@pytest.mark.parametrize("mut", pr.MUTATIONS)
def test_comparison_rejects_mutation(oracle, mut):
    for name in MUTANT_CASE[mut]:
        case = pr.get_case(name)
        with pytest.raises(pr.Mismatch):
            pr.compare(case, pr.simulate(case, mut))


def test_comparison_rejects_non_zero_padding_columns():
    case = pr.get_case("tail257")
    for v in (-0.0, 1e-300):
        got = pr.simulate(case)
        got["slab"][0, 1, 20] = v
        with pytest.raises(pr.Mismatch):
            pr.compare(case, got)


# ------------------------------------------------------------------ the margins hold -------
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_margins_hold_for_every_gpu_input(oracle, name):
    case = pr.get_case(name)
    info = pr.compare(case, pr.simulate(case))
    assert info["max_dq_ulp"] == 0
    S, P = case["limit"].shape
    assert np.all(np.isfinite(case["limit"]))
    n_read, offs, _, _ = sr.layout(case)
    for p in range(P):
        for s in range(S):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            with np.errstate(invalid="ignore"):
                k = case["d2"][s, sl] <= case["limit"][s, p]
            m = case["match"][s, sl][k]
            assert np.all((m >= 0) & (m < case["n_ref"][p]))


def test_cases_reach_what_they_are_for(oracle):
    got = pr.simulate(pr.get_case("none_kept"))
    assert got["status"][:, 0].tolist() == [1, 1] and got["iters"][1, 0] == 0
    got = pr.simulate(pr.get_case("nonrigid"))
    assert (got["status"][0, 0], got["iters"][0, 0], got["active"][0, 0]) == (5, 1, 0)
    for k in pr.RING_SMOOTH:
        got = pr.simulate(pr.get_case(f"ring{k}"))
        c = pr.RING_CONVERGES
        assert got["converged"][:, 0].tolist() == [0] * (c - 1) + [1] * (pr.RING_STEPS - c + 1), k
        assert got["hist_count"][-1, 0] == c + 1 > sr.RING and got["iters"][-1, 0] == c
    got = pr.simulate(pr.get_case("counter"))
    assert got["iters"][-1, 0] == 36 and got["converged"][-1, 0] == 0 and got["status"][-1, 0] == 0
    for n in pr.TAILS:
        got = pr.simulate(pr.get_case(f"tail{n}"))
        assert got["kept"][0].tolist() == [0, n // 2 + 1, n]


# ------------------------------------------------------------------ the entry's checks -----
def test_entry_rejects_bad_arguments_without_a_device():
    import aicp_mapping_amd._lib as L

    assert "aicp_hip_test_step_p2p" in L.EXPORTS and callable(L.Context.test_step_p2p)
    u32, i32, fl = C.c_uint32, C.c_int32, C.c_float
    inv = L.AICP_ERR_INVALID
    call = lambda **over: L.lib.aicp_hip_test_step_p2p(*pr.entry_args(**over)[0])
    for name in ("ctx", "n_read", "n_ref", "ref_off", "read_c", "ref_pts", "limit", "match", "d2", "touched",
                 "out_slab", "out_T", "out_state", "out_inlier", "out_touched", "out_dqdt", "out_dirty"):
        assert call(**{name: None}) == inv, name
    assert call(n_pairs=0) == inv and call(n_pairs=4097) == inv and call(n_steps=0) == inv
    assert call(n_read=(u32 * 1)(0)) == inv and call(n_ref=(u32 * 1)(0)) == inv
    assert call(ref_off=(u32 * 1)(1)) == inv and call(total_ref=0) == inv
    for smooth in (0, -1, 32):
        assert call(smooth=smooth) == inv, smooth
    for lim in (math.inf, -math.inf, math.nan):
        assert call(limit=(fl * 1)(lim)) == inv, lim
    for m in (-1, 2, 2 ** 31 - 1):
        assert call(match=(i32 * 2)(0, m)) == inv, m
    assert call(n_steps=2 ** 31) == inv and call(n_read=(u32 * 1)(2 ** 31)) == inv
    case = dict(pr.get_case("tail1"))
    case["match"] = case["match"][:, :-1]
    with pytest.raises(ValueError):
        L.Context.test_step_p2p(None, **case)
    assert L.default_config(point_to_point=True).knn_normals == 0 and L.default_config().knn_normals == 20
