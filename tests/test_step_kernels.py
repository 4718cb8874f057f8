"""The tail of every ICP iteration, k_icp_reduce and k_icp_update_f as launch_icp_reduce_f launches
them, against exact sums and a bit-exact restatement of the update.

Context.test_step (aicp_hip_test_step) runs the production launch on given matches with the ICP
loop's set-up; step_reference.compare checks what it returns: every slab row and every pair total
against math.fsum of the exact products within the derived bound (n + 2) 2^-53 sum|t|, the integer
columns, the sentinel in rows of inactive pairs, and T_iter, kept, iters, status, active, converged,
hist_count, inlier_ratio, the touch totals and dt bit for bit from the device's own rows (dq within
4 ulp: atan2). The inputs are step_reference.CASES; test_step_reference.py checks on the CPU that
each reaches what it is for and keeps the reference's margins.
"""
import ctypes as C

import numpy as np
import pytest

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
    case = sr.get_case(name)
    got = ctx.test_step(**case)
    info = sr.compare(case, got)   # (dirty == 0 is part of it)
    print(f"{name}: largest dq difference {info['max_dq_ulp']} ulp; solve6 paths {info['paths'][0]}")
    return got, info


@pytest.mark.parametrize("n", sr.TAILS)
def test_tails(ctx, n):
    """n_read on both sides of a block of 256 and of a row of 1024, none / half / all kept, matches
    at both ends of a shared reference."""
    got, _ = run(ctx, f"tail{n}")
    assert got["kept"][0].tolist() == [0, n // 2 + 1, n]
    assert got["status"][0].tolist() == [1, 0, 0]


def test_ties_and_non_finite_distances(ctx):
    case = sr.get_case("ties")
    got, _ = run(ctx, "ties")
    with np.errstate(invalid="ignore"):
        assert got["kept"][0, 0] == int((case["d2"][0] <= case["limit"][0, 0]).sum())


def test_ragged_batch(ctx):
    """Distinct ref_off and red_blk_off per pair; the pair that starts inactive keeps the sentinel
    (checked by compare) and its state; the two pairs with identical inputs agree bit for bit."""
    case = sr.get_case("ragged")
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
    case = sr.get_case("ragged")
    a, b = ctx.test_step(**case), ctx.test_step(**case)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_more_than_128_rows(ctx):
    """129 rows: the update's r0 loop runs a second pass; compare forms the totals in the documented
    order from the device's rows, so a row left out or added in another order changes T_iter."""
    case = sr.get_case("rows129")
    got, _ = run(ctx, "rows129")
    assert got["slab"].shape[1] == 129 and got["kept"][0, 0] == int((case["d2"][0] <= case["limit"][0, 0]).sum())


def test_touch_counters(ctx):
    got, _ = run(ctx, "touch")
    assert got["touched_pts"][-1, 0] > 2 ** 32 and got["touched_nodes"][-1, 0] > 2 ** 32


def test_solver_paths(ctx):
    """Systems of rank 6, 5, 3 and 1: the two-wave LLT path and the serial fall-back."""
    _, info = run(ctx, "ranks")
    assert info["paths"][0] == [0, 1, 1, 1]


def test_rank_threshold_family(ctx):
    """Normals z + s e across the 6 FLT_EPSILON rank threshold: T_iter equals the reference's on
    both sides (compare), whichever solve6 path the oracle takes on the device's totals."""
    _, info = run(ctx, "threshold")
    print("threshold family, s:", sr.THRESHOLD_S)
    print("threshold family, paths on the device's totals:", info["paths"])
    assert {0, 1} <= set(info["paths"][0])


def test_status_no_point_to_minimize(ctx):
    case = sr.get_case("none_kept")
    got, _ = run(ctx, "none_kept")
    assert got["status"][:, 0].tolist() == [1, 1] and got["active"][:, 0].tolist() == [0, 0]
    assert np.array_equal(got["T"][1, 0], case["init_T"]) and got["iters"][1, 0] == 0


def test_status_non_rigid_after_one_step(ctx):
    got, _ = run(ctx, "nonrigid")
    assert (got["status"][0, 0], got["iters"][0, 0], got["active"][0, 0]) == (5, 1, 0)
    assert (got["status"][1, 0], got["iters"][1, 0]) == (5, 1)


def test_status_nan_through_the_checker(ctx):
    """A NaN normal on a kept reference: the step itself goes through (a NaN determinant passes
    checkParameters), and the Differential checker's NaN branch stops the pair once hist_count
    exceeds smooth; every step is compared."""
    got, _ = run(ctx, "nan_normal")
    assert got["status"][:, 0].tolist() == [0, 1, 1, 1] and got["active"][:, 0].tolist() == [1, 0, 0, 0]


@pytest.mark.parametrize("smooth", sr.RING_SMOOTH)
def test_checker_ring_wraps(ctx, smooth):
    got, info = run(ctx, f"ring{smooth}")
    c = sr.RING_CONVERGES
    assert got["converged"][:, 0].tolist() == [0] * (c - 1) + [1] * (sr.RING_STEPS - c + 1)
    assert got["hist_count"][-1, 0] == c + 1 > sr.RING and got["iters"][-1, 0] == c


def test_counter_stops_at_max_iter(ctx):
    got, _ = run(ctx, "counter")
    assert got["active"][:, 0].tolist() == [1] * 35 + [0] * 5
    assert (got["iters"][-1, 0], got["converged"][-1, 0], got["status"][-1, 0]) == (36, 0, 0)


def test_rejected_calls_and_the_accepted_one(ctx, L):
    """The base call of test_step_reference's rejection test is accepted; an unkept reading may be
    unmatched; a kept one may not; the context serves a registration afterwards."""
    args, keep = sr.entry_args(ctx=ctx.h)
    assert L.lib.aicp_hip_test_step(*args) == L.AICP_OK
    assert keep["out_state"][0] == 2 and keep["out_state"][1] == 1   # kept, iters
    args, keep = sr.entry_args(ctx=ctx.h, match=(C.c_int32 * 2)(0, -1), d2=(C.c_float * 2)(0.5, 2.0))
    assert L.lib.aicp_hip_test_step(*args) == L.AICP_OK and keep["out_state"][0] == 1
    args, _ = sr.entry_args(ctx=ctx.h, match=(C.c_int32 * 2)(0, -1))
    assert L.lib.aicp_hip_test_step(*args) == L.AICP_ERR_INVALID
    case = dict(sr.get_case("tail257"))
    case["smooth"] = 32
    with pytest.raises(L.AicpError) as e:
        ctx.test_step(**case)
    assert e.value.code == L.AICP_ERR_INVALID
    from aicp_mapping_amd import synthetic as sy

    pr = sy.make_pair(3000, 3000, seed=3)
    T0, st0, rc0 = ctx.align_batch([dict(ref=pr.ref, read=pr.read)], flags=L.AICP_RUN_ICP)
    run(ctx, "tail1025")
    T1, st1, rc1 = ctx.align_batch([dict(ref=pr.ref, read=pr.read)], flags=L.AICP_RUN_ICP)
    assert rc0 == rc1 == 0 and np.array_equal(T0, T1) and st0[0]["iterations"] == st1[0]["iterations"]
