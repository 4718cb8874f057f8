"""The reference of test_step_kernels.py, checked on the CPU: it reproduces oracle.icp when a whole
registration is driven through it, its comparison rejects each of a set of plausible kernel bugs,
and the margins it needs (sin / cos away from float rounding boundaries, the smoothed differences
away from the thresholds) hold for every input the GPU tests run. Plus the argument checks of
aicp_hip_test_step, which all come before any device work.
"""
import ctypes as C
import math

import numpy as np
import pytest

import step_reference as sr
from aicp_mapping_amd import synthetic as sy

f32 = np.float32


# ------------------------------------------------------------------ 1. the reference is right
def _mean_fixed40(x):
    """The oracle's order-free centroid: coordinates rounded to multiples of 2^-40, summed exactly."""
    acc = sum(int(np.rint(np.float64(v) * 1099511627776.0)) for v in x)
    assert abs(acc) < 2 ** 64                 # one word: |S| as a double is a single rounding
    m = float(abs(acc)) * (1.0 / 1099511627776.0) / float(len(x))
    return f32(-m if acc < 0 else m)


def register(oracle, ref, read, ratio, max_iter=20, smooth=4, min_rot=1e-3, min_trans=1e-2):
    """ICP::compute with the reference step: normals on the raw reference, the centred matcher tree,
    kNN with eps 3.16, the trimmed limit, then sr.update on the exactly summed terms."""
    nrm, _, _ = oracle.surface_normals(ref, 20)
    mean = np.array([_mean_fixed40(ref[:, d]) for d in range(3)], f32)
    refc = (ref[:, :3] - mean).astype(f32)
    tree = oracle.Tree(refc, 8)
    Tinit = sr.ident16()
    Tinit[12:15] = -mean
    rd = sr.apply_points(Tinit, read[:, :3])
    st = sr.State()
    prm = dict(max_iter=max_iter, smooth=smooth, min_rot=min_rot, min_trans=min_trans)
    n = len(rd)
    while st.active:
        step = sr.apply_points(st.T, rd)
        ids, d2, _, _ = tree.knn(step, 1, 3.16)
        ids, d2 = ids[:, 0], d2[:, 0]
        limit, err = oracle.dists_quantile(d2[d2 != np.inf], ratio)
        assert err == 0
        case = dict(n_read=[n], n_ref=[len(refc)], ref_off=[0], read_c=rd, ref_pts=refc, ref_nrm=nrm,
                    limit=np.array([[limit]], f32), match=ids[None], d2=d2[None], touched=np.zeros((1, n), np.uint32))
        idx, prod, tp, tn = sr.pair_terms(case, 0, 0, st.T, f32(limit))
        tot = np.zeros(sr.COLS)
        tot[:27] = [math.fsum(prod[:, c].tolist()) for c in range(27)]
        tot[27] = len(idx)
        sr.update(st, tot, n, prm)
    Tmean = sr.ident16()
    Tmean[12:15] = mean
    T = sr.mul4(sr.mul4(Tmean, st.T), Tinit)
    return T.reshape(4, 4).T.copy(), st


@pytest.mark.parametrize("seed,n,ratio", [(5, 8000, 0.358818), (1, 20000, 0.6)])
def test_reference_registration_matches_oracle(oracle, seed, n, ratio):
    pr = sy.make_pair(n, n, seed=seed)
    rc, T1, st1 = oracle.icp(pr.ref, pr.read, oracle.default_config(trimmed_ratio=ratio, normals_on_centered=0))
    T, st = register(oracle, np.ascontiguousarray(pr.ref, f32), np.ascontiguousarray(pr.read, f32), ratio)
    assert rc == 0 and st.status == 0
    assert (st.iters, st.converged) == (st1.iterations, st1.converged)
    r, t = sy.rot_err(T1, T)
    assert r < 1e-6 and t < 1e-5, (r, t)
    assert st.inlier_ratio == f32(st1.inlier_ratio)


# ------------------------------------------------------------------ 2. the comparison is sharp
MUTANT_CASE = dict(lt="ties", drop_tail="tail1025", ref_off="ragged", swapF="tail257", rows128="rows129",
                   ring="ring4", fullrank="ranks")


def test_every_mutation_has_a_case():
    assert set(MUTANT_CASE) == set(sr.MUTATIONS)


@pytest.mark.parametrize("mut", sr.MUTATIONS)
def test_comparison_rejects_mutation(oracle, mut):
    """Outputs made by the reference with one bug built in are rejected; the unmutated reference's
    own outputs pass the same comparison (test_margins_hold_for_every_gpu_input)."""
    case = sr.get_case(MUTANT_CASE[mut])
    bad = sr.simulate(case, mut)
    with pytest.raises(sr.Mismatch):
        sr.compare(case, bad)


def test_ties_case_has_ties_on_both_sides():
    case = sr.get_case("ties")
    d2, lim = case["d2"][0], case["limit"][0, 0]
    assert (d2 == lim).sum() == 100 and (d2 == np.nextafter(lim, f32(np.inf))).sum() == 50
    assert np.isinf(d2).sum() == 20 and np.isnan(d2).sum() == 20
    got = sr.simulate(case)
    assert got["kept"][0, 0] == (d2 <= lim).sum() > (d2 < lim).sum() + 99


# ------------------------------------------------------------------ 3. the margins hold -----
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_margins_hold_for_every_gpu_input(oracle, name):
    """Building and simulating the case raises MarginError where a margin fails; the reference's
    own outputs pass its comparison, and the entry would accept the input."""
    case = sr.get_case(name)
    info = sr.compare(case, sr.simulate(case))
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
    """The solver paths, statuses and checker decisions each case exists to reach."""
    path = lambda name: sr.compare(sr.get_case(name), sr.simulate(sr.get_case(name)))["paths"]
    p = path("ranks")
    assert p[0][0] == 0 and all(p[0][k] in (1, 2) for k in (1, 2, 3)), p
    got = sr.simulate(sr.get_case("ranks"))
    assert got["kept"][0, 3] == 1
    # the threshold family reaches the rank-deficient paths and the LLT path, in that order of s
    t = path("threshold")[0]
    assert 0 in t and 1 in t, t
    assert t[0] == 1 and t[-1] == 0 and t == sorted(t, key=lambda v: (v + 2) % 3), t   # 1.., 2.., 0..
    k = t.index(0)
    assert 4 <= k - 1 and k <= 10, t   # the rank changes inside the fine steps around the threshold
    got = sr.simulate(sr.get_case("none_kept"))
    assert got["status"][:, 0].tolist() == [1, 1] and got["active"][0, 0] == 0 and got["iters"][1, 0] == 0
    assert np.array_equal(got["T"][1, 0], sr.get_case("none_kept")["init_T"])
    got = sr.simulate(sr.get_case("nonrigid"))
    assert (got["status"][0, 0], got["iters"][0, 0], got["active"][0, 0]) == (5, 1, 0)
    got = sr.simulate(sr.get_case("nan_normal"))   # hist_count > smooth = 2 at the second step
    assert got["status"][:, 0].tolist() == [0, 1, 1, 1] and got["active"][:, 0].tolist() == [1, 0, 0, 0]
    assert got["hist_count"][1, 0] == 3
    for k in sr.RING_SMOOTH:
        got = sr.simulate(sr.get_case(f"ring{k}"))
        c = sr.RING_CONVERGES
        assert got["converged"][:, 0].tolist() == [0] * (c - 1) + [1] * (sr.RING_STEPS - c + 1), k
        assert got["active"][:, 0].tolist() == [1] * (c - 1) + [0] * (sr.RING_STEPS - c + 1), k
        assert got["hist_count"][-1, 0] == c + 1 > sr.RING and got["iters"][-1, 0] == c
    got = sr.simulate(sr.get_case("counter"))
    assert got["iters"][-1, 0] == 36 and got["converged"][-1, 0] == 0 and got["status"][-1, 0] == 0
    assert got["active"][:, 0].tolist() == [1] * 35 + [0] * 5
    got = sr.simulate(sr.get_case("touch"))
    assert got["touched_pts"][-1, 0] > 2 ** 32 and got["touched_nodes"][-1, 0] > 2 ** 32
    got = sr.simulate(sr.get_case("ragged"))
    assert got["active"][:, 2].tolist() == [0, 0] and got["kept"][1, 2] == 0
    case = sr.get_case("ragged")
    assert len(set(case["ref_off"])) == 6 and len(set(sr.layout(case)[3][:-1].tolist())) == 6
    for n in sr.TAILS:
        got = sr.simulate(sr.get_case(f"tail{n}"))
        assert got["kept"][0].tolist() == [0, n // 2 + 1, n]


# ------------------------------------------------------------------ 4. the entry's checks ---
@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


def test_entry_rejects_bad_arguments_without_a_device(L):
    """Each rejected call differs from an accepted one in a single argument. (That the base call is
    accepted is checked where there is a device, in test_step_kernels.py.)"""
    assert "aicp_hip_test_step" in L.EXPORTS and callable(L.Context.test_step)
    u32, i32, fl = C.c_uint32, C.c_int32, C.c_float
    inv = L.AICP_ERR_INVALID
    call = lambda **over: L.lib.aicp_hip_test_step(*sr.entry_args(**over)[0])
    for name in ("ctx", "n_read", "n_ref", "ref_off", "read_c", "ref_pts", "ref_nrm", "limit", "match", "d2",
                 "touched", "out_slab", "out_T", "out_state", "out_inlier", "out_touched", "out_dqdt", "out_dirty"):
        assert call(**{name: None}) == inv, name
    assert call(n_pairs=0) == inv
    assert call(n_pairs=4097) == inv        # more than kMaxPairs (rejected before any array is read)
    assert call(n_steps=0) == inv
    assert call(n_read=(u32 * 1)(0)) == inv
    assert call(n_ref=(u32 * 1)(0)) == inv
    assert call(ref_off=(u32 * 1)(1)) == inv   # ref_off + n_ref above total_ref
    assert call(total_ref=0) == inv
    for smooth in (0, -1, 32):
        assert call(smooth=smooth) == inv, smooth
    for lim in (math.inf, -math.inf, math.nan):
        assert call(limit=(fl * 1)(lim)) == inv, lim
    for m in (-1, 2, 2 ** 31 - 1):
        assert call(match=(i32 * 2)(0, m)) == inv, m
    assert call(n_steps=2 ** 31) == inv             # n_steps * total = 2^32 (rejected before any array is walked)
    assert call(n_read=(u32 * 1)(2 ** 31)) == inv   # 2^31 readings


def test_wrapper_rejects_ragged_arrays(L):
    case = dict(sr.get_case("tail1"))
    case["match"] = case["match"][:, :-1]
    with pytest.raises(ValueError):
        L.Context.test_step(None, **case)
