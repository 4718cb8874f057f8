"""The tail of a point-to-point ICP iteration, k_icp_reduce_p2p and k_icp_update_p2p as
launch_icp_reduce_f launches them for knn_normals == 0, against exact sums and a bit-exact
restatement of the update.

Context.test_step_p2p (aicp_hip_test_step_p2p) runs the production launch on given matches with the
ICP loop's set-up; p2p_reference.compare checks what it returns: every slab row and pair total
against math.fsum of the exact terms within (n + 2) 2^-53 sum|t|, columns 15..26 exactly +0.0, the
integer columns, the sentinel in rows of inactive pairs, and T_iter, kept, iters, status, active,
converged, hist_count, inlier_ratio, the touch totals and dt bit for bit from the device's own rows
(dq within 4 ulp: atan2). The inputs are p2p_reference.CASES; test_p2p_reference.py checks on the
CPU that each reaches what it is for and keeps the reference's margins.
"""
import numpy as np
import pytest

import p2p_reference as pr
import step_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def run(ctx, name):
    """One case on the device against the reference; returns (got, info)."""
    case = pr.get_case(name)
    got = ctx.test_step_p2p(**case)
    info = pr.compare(case, got)   # (dirty == 0 is part of it)
    print(f"{name}: largest dq difference {info['max_dq_ulp']} ulp; ranks {info['ranks'][0]}")
    return got, info


@pytest.mark.parametrize("n", pr.TAILS)
def test_tails(ctx, n):
    """n_read on both sides of a block of 256 and of a row of 1024, none / half / all kept."""
    got, _ = run(ctx, f"tail{n}")
    assert got["kept"][0].tolist() == [0, n // 2 + 1, n]
    assert got["status"][0].tolist() == [1, 0, 0]


def test_ties_and_non_finite_distances(ctx):
    case = pr.get_case("ties")
    got, _ = run(ctx, "ties")
    with np.errstate(invalid="ignore"):
        assert got["kept"][0, 0] == int((case["d2"][0] <= case["limit"][0, 0]).sum())


def test_ragged_batch(ctx):
    """Distinct ref_off and red_blk_off per pair; the pair that starts inactive keeps the sentinel
    (checked by compare) and its state; the two pairs with identical inputs agree bit for bit."""
    case = pr.get_case("ragged")
    got, _ = run(ctx, "ragged")
    _, _, _, roff = sr.layout(case)
    for s in range(2):
        assert (got["active"][s, 2], got["iters"][s, 2], got["hist_count"][s, 2], got["kept"][s, 2]) == (0, 0, 1, 0)
        assert np.array_equal(got["T"][s, 2], sr.ident16())
        a = got["slab"][s, roff[1]:roff[2]].view(np.uint64)
        b = got["slab"][s, roff[5]:roff[6]].view(np.uint64)
        assert np.array_equal(a, b)
        for k in ("T", "inlier_ratio", "dq", "dt"):
            assert got[k][s, 1].tobytes() == got[k][s, 5].tobytes(), k
        for k in sr.INT_KEYS + ("touched_pts", "touched_nodes"):
            assert got[k][s, 1] == got[k][s, 5], k


def test_ragged_batch_is_deterministic(ctx):
    case = pr.get_case("ragged")
    a, b = ctx.test_step_p2p(**case), ctx.test_step_p2p(**case)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a["dirty"] == 0


def test_more_than_128_rows(ctx):
    case = pr.get_case("rows129")
    got, _ = run(ctx, "rows129")
    assert got["slab"].shape[1] == 129 and got["kept"][0, 0] == int((case["d2"][0] <= case["limit"][0, 0]).sum())


def test_exact_correspondences(ctx):
    got, info = run(ctx, "exact")
    assert info["ranks"][0] == [3] and got["kept"][0, 0] == 300
    T = got["T"][0, 0].reshape(4, 4).T.astype(np.float64)
    assert np.abs(T[:3, :3] - pr.EXACT_R).max() < 2e-7 and np.abs(T[:3, 3] - pr.EXACT_T).max() < 1e-6


def test_reflection(ctx):
    """det(U V^T) < 0 on the device's own totals; the step's rotation is proper."""
    got, info = run(ctx, "reflection")
    assert info["ranks"][0] == [3] and got["status"][:, 0].tolist() == [0, 0]
    tot = pr.total_from_rows(got["slab"][0])
    Un, _, Vtn = np.linalg.svd(np.array(pr.cross_covariance(tot)[2]))
    assert np.linalg.det(Un @ Vtn) < 0
    assert np.linalg.det(got["T"][0, 0].reshape(4, 4).T[:3, :3].astype(np.float64)) > 0.999


def test_ranks(ctx):
    """General, planar (rank 2: the cross products), collinear and single-point (R = I) pairs."""
    got, info = run(ctx, "ranks")
    assert tuple(info["ranks"][0]) == pr.RANKS and got["kept"][0, 3] == 1
    for p in (2, 3):
        assert np.array_equal(got["T"][0, p].reshape(4, 4).T[:3, :3], np.eye(3, dtype=np.float32))


def test_rank_threshold_family(ctx):
    _, info = run(ctx, "threshold")
    print("threshold family, z:", pr.THRESHOLD_Z)
    print("threshold family, ranks on the device's totals:", info["ranks"])
    assert {2, 3} <= set(info["ranks"][0])


def test_status_no_point_to_minimize(ctx):
    case = pr.get_case("none_kept")
    got, _ = run(ctx, "none_kept")
    assert got["status"][:, 0].tolist() == [1, 1] and got["active"][:, 0].tolist() == [0, 0]
    assert np.array_equal(got["T"][1, 0], case["init_T"]) and got["iters"][1, 0] == 0


def test_status_non_rigid_after_one_step(ctx):
    got, _ = run(ctx, "nonrigid")
    assert (got["status"][0, 0], got["iters"][0, 0], got["active"][0, 0]) == (5, 1, 0)
    assert (got["status"][1, 0], got["iters"][1, 0]) == (5, 1)


@pytest.mark.parametrize("smooth", pr.RING_SMOOTH)
def test_checker_ring_wraps(ctx, smooth):
    got, _ = run(ctx, f"ring{smooth}")
    c = pr.RING_CONVERGES
    assert got["converged"][:, 0].tolist() == [0] * (c - 1) + [1] * (pr.RING_STEPS - c + 1)
    assert got["hist_count"][-1, 0] == c + 1 > sr.RING and got["iters"][-1, 0] == c


def test_counter_stops_at_max_iter(ctx):
    got, _ = run(ctx, "counter")
    assert got["active"][:, 0].tolist() == [1] * 35 + [0] * 5
    assert (got["iters"][-1, 0], got["converged"][-1, 0], got["status"][-1, 0]) == (36, 0, 0)


def test_accepted_calls_and_the_context_afterwards(ctx, L):
    """The base call of the CPU rejection test is accepted; an unkept reading may be unmatched, a kept
    one may not; the point-to-plane entry and a registration work on the same context afterwards."""
    import ctypes as C

    args, keep = pr.entry_args(ctx=ctx.h)
    assert L.lib.aicp_hip_test_step_p2p(*args) == L.AICP_OK
    assert keep["out_state"][0] == 2 and keep["out_state"][1] == 1   # kept, iters
    args, keep = pr.entry_args(ctx=ctx.h, match=(C.c_int32 * 2)(0, -1), d2=(C.c_float * 2)(0.5, 2.0))
    assert L.lib.aicp_hip_test_step_p2p(*args) == L.AICP_OK and keep["out_state"][0] == 1
    args, _ = pr.entry_args(ctx=ctx.h, match=(C.c_int32 * 2)(0, -1))
    assert L.lib.aicp_hip_test_step_p2p(*args) == L.AICP_ERR_INVALID
    case = sr.get_case("tail257")
    sr.compare(case, ctx.test_step(**case))   # the point-to-plane kernels, picked by the same launch
    run(ctx, "tail257")
