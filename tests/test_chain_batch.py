"""The sampled chains in batches on the GPU (aicp_hip_align_chain_batch).

1 the filters over ragged batches (aicp_hip_test_chain_batch) against the numpy reference cloud by
  cloud, and against aicp_hip_chain_filter on each cloud alone, bit for bit;
2 whole runs: every pair of a batch gets the one-pair call's bits and statistics, in any order;
3 shared references; 4 the overlap form (App's order); 5 emptied sides; 6 the plain chain.
Every comparison is exact.
"""
import functools

import numpy as np
import pytest

import chain_batch_reference as cb
import chain_reference as cr
from aicp_mapping_amd import synthetic as sy

f32 = np.float32
gpu = pytest.mark.gpu
STAT_FIELDS = ("status", "iterations", "converged", "inlier_ratio", "trimmed_ratio", "degenerate_normals")


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one(L):
    """The context of the one-pair calls the batch is compared with."""
    c = L.Context(0)
    c.set_options(reference_cache=0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1: the filters ----------
@gpu
@pytest.mark.parametrize("name", sorted(cb.cases()))
def test_filters_over_a_ragged_batch(ctx, one, L, name):
    case = cb.cases()[name]
    side = case["side"]
    ch = cr.make_chain(L, case["filters"] if side == cr.REFERENCE else (), case["filters"] if side == cr.READING else (),
                       seed=case["seed"])
    nrm, dens = cb.has_normals(case), cb.has_densities(case)
    got = ctx.test_chain_batch(ch, side, case["clouds"], normals=nrm, densities=dens)
    assert len(got) == len(case["clouds"])
    # the numpy reference, on the device's own densities: counts and indices exactly
    bad = cb.mismatches(case, got, [g["densities"] for g in got] if dens else None)
    assert bad == [], bad
    # the one-pair filter on each cloud alone: indices, normals and densities bit for bit
    for c, (pts, g) in enumerate(zip(case["clouds"], got)):
        alone = one.chain_filter(ch, side, pts, densities=dens, normals=nrm)
        assert alone["n"] == g["n"] and alone["counts"] == g["counts"], (c, alone["counts"], g["counts"])
        assert np.array_equal(alone["index"], g["index"]), c
        if nrm:
            assert alone["normals"].tobytes() == g["normals"].tobytes(), c
        if dens:
            assert alone["densities"].tobytes() == g["densities"].tobytes(), c
    print(name, [g["counts"] for g in got])


# ------------------------------------------------------------------ whole runs: set-up -------
def plane_cfg(L, ratio=0.75):
    return L.default_config(knn_normals=10, nn_epsilon=0.0, trimmed_ratio=ratio, max_iter=100, min_diff_rot=0.001,
                            min_diff_trans=0.001, smooth_length=4)


def p2p_cfg(L, ratio=0.75):
    return L.default_config(point_to_point=True, nn_epsilon=3.16, trimmed_ratio=ratio, max_iter=150, min_diff_rot=0.001,
                            min_diff_trans=0.01, smooth_length=4)


BESL = (dict(kind=cr.MIN_DIST, dim=-1, min_dist=1.0), dict(kind=cr.RANDOM, prob=0.5))
REF_3D = (dict(kind=cr.SN, knn=10, keep_densities=0), dict(kind=cr.RANDOM, prob=0.5))
READ_3D = (dict(kind=cr.SN, knn=10, keep_densities=1), dict(kind=cr.MAX_DENSITY, max_density=3.75))
# name -> (config, reference list, reading list, MaxDist limit on d2 or None)
SHAPES = dict(besl92=(p2p_cfg, BESL, BESL, None), trimmed=(plane_cfg, REF_3D, READ_3D, None),
              max=(plane_cfg, REF_3D, READ_3D, 0.15))


@functools.lru_cache(maxsize=None)
def scene(n, seed):
    p = sy.make_pair(n, n, seed=seed, half=12.0)
    return dict(ref=np.ascontiguousarray(p.ref, f32), read=np.ascontiguousarray(p.read, f32),
                ref_origin=tuple(p.ref_origin), read_origin=tuple(p.read_origin))


def near(n, seed):
    """n points inside MinDist's unit sphere (which empties the cloud) and dense enough that every
    one lies above maxDensity 3.75 and, for the cube, is saturated (which empties it too)."""
    return (np.random.default_rng(seed).uniform(-0.2, 0.2, (n, 3))).astype(f32)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Scene pairs of 2-4 k points, a pair of 6 points (too small for SurfaceNormal's 10 neighbours), a
    one-point reading, and a reading every filter list here empties: inside MinDist's radius, and a
    small cube whose points are all saturated above maxDensity."""
    a, b, c, d = scene(3000, 7), scene(2048, 8), scene(3500, 9), scene(2500, 10)
    tiny = dict(ref=np.ascontiguousarray(a["ref"][:6]), read=np.ascontiguousarray(a["read"][:6]))
    lone = dict(ref=b["ref"], read=np.ascontiguousarray(c["read"][:1]))
    emptied = dict(ref=c["ref"], read=(cr.CUBE8 * f32(0.25)).astype(f32))
    return [a, tiny, b, emptied, c, lone, d]


def strip(pairs):
    return [dict(ref=p["ref"], read=p["read"]) for p in pairs]


def check_pair(one, L, cfg, ch, pr, T, st, cs, tag):
    """Pair `pr` of a batch against the one-pair call: bits, statistics, every chain_stats field."""
    T1, st1, cs1, rc1 = one.register_chain(pr["ref"], pr["read"], cfg, ch, raise_on_error=False)
    assert st["status"] == rc1 == st1["status"], (tag, st["status"], rc1)
    if min(cs1["n_kept"]) == 0:   # an emptied side: the one-pair call leaves out_T alone, the batch writes the identity
        assert rc1 == L.AICP_ERR_CONVERGENCE and T.tobytes() == np.eye(4, dtype=f32).tobytes(), (tag, T)
    else:
        assert T.tobytes() == T1.tobytes(), (tag, T, T1)
    for k in STAT_FIELDS:
        assert st[k] == st1[k], (tag, k, st[k], st1[k])
    assert cs == cs1, (tag, cs, cs1)
    return rc1


# ------------------------------------------------------------------ 2: whole runs -----------
@gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_pair_of_a_batch_gets_the_one_pair_bits(ctx, one, L, shape):
    mk, rf, df, lim = SHAPES[shape]
    cfg = mk(L)
    ch = cr.make_chain(L, rf, df, seed=5, max_dist_d2=lim)
    pairs = strip(mixed_batch())
    T, st, cs, rc = ctx.align_chain_batch(pairs, cfg, ch, raise_on_error=False)
    rcs = [check_pair(one, L, cfg, ch, pairs[i], T[i], st[i], cs[i], (shape, i)) for i in range(len(pairs))]
    print(shape, "statuses", rcs, "iterations", [s["iterations"] for s in st], "kept", [c["n_kept"] for c in cs])
    assert rc == next((r for r in rcs if r), 0)
    assert rcs[3] == L.AICP_ERR_CONVERGENCE and cs[3]["n_kept"][1] == 0   # the emptied reading
    assert sum(1 for r in rcs if r == 0) >= 4 and all(st[i]["iterations"] > 0 for i in (0, 2, 4, 6))
    # the same batch reversed, and a one-pair slice of it
    Tr, str_, csr, _ = ctx.align_chain_batch(pairs[::-1], cfg, ch, raise_on_error=False)
    n = len(pairs)
    for i in range(n):
        assert Tr[n - 1 - i].tobytes() == T[i].tobytes() and csr[n - 1 - i] == cs[i], (shape, i)
        assert all(str_[n - 1 - i][k] == st[i][k] for k in STAT_FIELDS), (shape, i)
    for i in (2, 1):
        Ts, sts, css, _ = ctx.align_chain_batch(pairs[i:i + 1], cfg, ch, raise_on_error=False)
        assert Ts[0].tobytes() == T[i].tobytes() and css[0] == cs[i], (shape, i)
        assert all(sts[0][k] == st[i][k] for k in STAT_FIELDS), (shape, i)


# ------------------------------------------------------------------ 3: shared references ----
@gpu
@pytest.mark.parametrize("shape", ["besl92", "trimmed"])
def test_two_references_times_three_readings(ctx, one, L, shape):
    mk, rf, df, lim = SHAPES[shape]
    cfg = mk(L)
    ch = cr.make_chain(L, rf, df, seed=9, max_dist_d2=lim)
    a, b, c = scene(3000, 7), scene(2048, 8), scene(2500, 10)
    refs = [a["ref"], np.ascontiguousarray(a["read"][:2777])]
    reads = [a["read"], np.ascontiguousarray(a["ref"][100:2600]), np.ascontiguousarray(a["read"][::-1][:2222])]
    pairs = [dict(ref=r, read=d) for d in reads for r in refs]   # the references alternate
    T, st, cs, rc = ctx.align_chain_batch(pairs, cfg, ch, raise_on_error=False)
    for i, pr in enumerate(pairs):
        check_pair(one, L, cfg, ch, pr, T[i], st[i], cs[i], (shape, i))
    assert rc == 0 and all(s["iterations"] > 0 for s in st)
    # (two references' counts, each shared by three pairs)
    assert len({tuple(c["n_out"][0]) for c in cs}) == 2 and cs[0]["n_out"][0] == cs[2]["n_out"][0] == cs[4]["n_out"][0]


# ------------------------------------------------------------------ 4: the overlap form -----
@gpu
@pytest.mark.parametrize("shape", ["trimmed", "max"])
def test_overlap_form_is_apps_order(ctx, one, L, shape):
    mk, rf, df, lim = SHAPES[shape]
    ch = cr.make_chain(L, rf, df, seed=5, max_dist_d2=lim)
    a, b, c = scene(3000, 7), scene(2048, 8), scene(2500, 10)
    pairs = [a, b, dict(a, read=b["read"], read_origin=b["read_origin"]), c]
    res = float(f32(0.2))
    flags = L.AICP_RUN_ICP | L.AICP_RUN_OVERLAP
    # (cfg.trimmed_ratio is not read: a value the auto-tuned ratios do not take)
    T, st, cs, rc = ctx.align_chain_batch(pairs, mk(L, 0.123), ch, resolution=res, flags=flags, raise_on_error=False)
    _, sto, _ = one.align_batch(pairs, mk(L), resolution=res, flags=L.AICP_RUN_OVERLAP)
    ratios, rcs = set(), []
    for i, pr in enumerate(pairs):
        assert st[i]["overlap_percent"] == sto[i]["overlap_percent"] and st[i]["overlap_keys"] == sto[i]["overlap_keys"], i
        assert st[i]["overlap_percent"] > 0
        ratio = L.autotune_ratio(st[i]["overlap_percent"])
        assert st[i]["trimmed_ratio"] == f32(ratio), (i, st[i]["trimmed_ratio"], ratio)
        ratios.add(ratio)
        T1, st1, cs1, rc1 = one.register_chain(pr["ref"], pr["read"], mk(L, ratio), ch, raise_on_error=False)
        rcs.append(rc1)
        assert T[i].tobytes() == T1.tobytes(), (shape, i)
        assert cs[i] == cs1 and all(st[i][k] == st1[k] for k in STAT_FIELDS if k != "trimmed_ratio"), (shape, i)
    print(shape, "overlap", [s["overlap_percent"] for s in st], "ratios", sorted(ratios), "statuses", rcs)
    assert rc == next((r for r in rcs if r), 0) and rcs[0] == rcs[1] == rcs[3] == 0 and len(ratios) > 1, (rcs, ratios)
    # the flags the call takes
    for bad in (0, L.AICP_RUN_OVERLAP, flags | L.AICP_RUN_TIME_NN):
        assert ctx.align_chain_batch(pairs, mk(L), ch, resolution=res, flags=bad, raise_on_error=False)[3] == L.AICP_ERR_INVALID
    assert ctx.align_chain_batch(pairs, mk(L), ch, resolution=0.0, flags=flags, raise_on_error=False)[3] == L.AICP_ERR_INVALID


# ------------------------------------------------------------------ 5: emptied sides --------
@gpu
def test_emptied_sides_end_their_pairs_alone(ctx, one, L):
    cfg = p2p_cfg(L)
    ch = cr.make_chain(L, BESL, BESL, seed=4)
    a, b, c = scene(3000, 7), scene(2048, 8), scene(2500, 10)
    gone = near(300, 1)        # a reference that MinDist empties, shared by two pairs
    pairs = [dict(ref=a["ref"], read=a["read"]),
             dict(ref=b["ref"], read=near(200, 2)),          # 1: its reading emptied
             dict(ref=b["ref"], read=b["read"]),
             dict(ref=near(100, 3), read=c["read"]),         # 3: its reference emptied
             dict(ref=gone, read=a["read"]),                 # 4, 6: the shared reference emptied
             dict(ref=c["ref"], read=c["read"]),
             dict(ref=gone, read=b["read"]),
             dict(ref=a["ref"], read=b["read"])]
    T, st, cs, rc = ctx.align_chain_batch(pairs, cfg, ch, raise_on_error=False)
    err = ctx.last_error()
    dead = {1: "reading", 3: "reference", 4: "reference", 6: "reference"}
    eye = np.eye(4, dtype=f32)
    for i, pr in enumerate(pairs):
        check_pair(one, L, cfg, ch, pr, T[i], st[i], cs[i], i)
        if i in dead:
            assert st[i]["status"] == L.AICP_ERR_CONVERGENCE and T[i].tobytes() == eye.tobytes(), i
            assert cs[i]["n_kept"][0 if dead[i] == "reference" else 1] == 0, (i, cs[i])
        else:
            assert st[i]["status"] == 0 and st[i]["iterations"] > 0 and min(cs[i]["n_kept"]) > 500, (i, st[i])
    # the return value and the text are the first failing pair's, in pair order
    assert rc == L.AICP_ERR_CONVERGENCE
    assert err.startswith("pair 1:") and "the chain's filters leave no point of the reading" in err, err
    with pytest.raises(L.ConvergenceError):
        ctx.align_chain_batch(pairs, cfg, ch)
    # with the reference's pairs first, the text names the reference
    T2, st2, cs2, rc2 = ctx.align_chain_batch(pairs[3:], cfg, ch, raise_on_error=False)
    err2 = ctx.last_error()
    assert rc2 == L.AICP_ERR_CONVERGENCE and err2.startswith("pair 0:") and "no point of the reference" in err2, err2
    for k in range(len(pairs) - 3):
        assert T2[k].tobytes() == T[3 + k].tobytes() and cs2[k] == cs[3 + k], k
    # every pair emptied: nothing runs, every status is set
    T3, st3, _, rc3 = ctx.align_chain_batch([pairs[1], pairs[4]], cfg, ch, raise_on_error=False)
    assert rc3 == L.AICP_ERR_CONVERGENCE and [s["status"] for s in st3] == [L.AICP_ERR_CONVERGENCE] * 2
    assert T3[0].tobytes() == T3[1].tobytes() == eye.tobytes()


# ------------------------------------------------------------------ 6: the plain chain -------
@gpu
@pytest.mark.parametrize("flags", ["icp", "icp_overlap"])
def test_plain_chain_gives_the_bits_of_align_batch(ctx, one, L, flags):
    a, b, c = scene(3000, 7), scene(2048, 8), scene(2500, 10)
    pairs = [a, b, c]
    cfg = plane_cfg(L)
    fl = L.AICP_RUN_ICP | (L.AICP_RUN_OVERLAP if flags == "icp_overlap" else 0)
    res = float(f32(0.2))
    T0, st0, rc0 = one.align_batch(pairs, cfg, resolution=res, flags=fl)
    sn = cr.make_chain(L, [dict(kind=cr.SN, knn=10)], [dict(kind=cr.SN, knn=10, keep_densities=1)])
    for ch in (L.Chain(), sn):
        T, st, cs, rc = ctx.align_chain_batch(pairs, cfg, ch, resolution=res, flags=fl)
        assert rc == rc0 == 0 and T.tobytes() == T0.tobytes() and st == st0
        assert [c_["n_kept"] for c_ in cs] == [[len(p["ref"]), len(p["read"])] for p in pairs]
        assert all(c_["n_out"][0][:ch.n_filters[0]] == [len(p["ref"])] * ch.n_filters[0] for c_, p in zip(cs, pairs))


# ------------------------------------------------------------------ 7: the one-pair corner ---
@gpu
def test_one_pair_call_passes_a_cloud_emptied_in_front_of_surface_normal_and_max_density(one, L):
    """A cloud that MinDist empties in front of a SurfaceNormal -> MaxDensity tail is AICP_OK with 0
    points in aicp_hip_chain_filter, as its header says of emptied clouds (no point reaches the
    SurfaceNormal, so there are no densities and nothing for MaxDensity to drop), and the side left
    without a point in aicp_hip_register_chain: the answers a batch gives such a pair."""
    fl = cb.cases()["mindist_density"]["filters"]
    inside = cb.cases()["mindist_density"]["clouds"][1]      # every point within MinDist's 2 m
    ch = cr.make_chain(L, (), fl, seed=21)
    got = one.chain_filter(ch, cr.READING, inside, densities=True)
    assert got["n"] == 0 and got["counts"] == [0, 0, 0] and len(got["index"]) == 0 and len(got["densities"]) == 0
    a = scene(2048, 8)
    T, st, cs, rc = one.register_chain(a["ref"], inside, plane_cfg(L), ch, raise_on_error=False)
    assert rc == L.AICP_ERR_CONVERGENCE and "reading" in one.last_error() and cs["n_kept"] == [2048, 0]
    # a cloud with points is filtered as before
    full = one.chain_filter(ch, cr.READING, cb.cases()["mindist_density"]["clouds"][0], densities=True)
    assert full["counts"] == [587, 587, 477]


# ------------------------------------------------------------------ 8: the argument codes ----
@gpu
def test_argument_checks_of_the_batch_call(ctx, L):
    import ctypes as C

    a = scene(2048, 8)
    cfg, ch = p2p_cfg(L), cr.make_chain(L, BESL, BESL, seed=4)
    p, keep = L.make_pair(a["ref"], a["read"])
    T = np.zeros(16, f32)

    def call(pairs=p, n=1, out=T, cfg_=cfg, ch_=ch, flags=L.AICP_RUN_ICP):
        return L.lib.aicp_hip_align_chain_batch(ctx.h, C.byref(cfg_) if cfg_ is not None else None,
                                                C.byref(ch_) if ch_ is not None else None,
                                                C.byref(pairs) if pairs is not None else None, n, 0.2, flags,
                                                L._fptr(out) if out is not None else None, None, None)

    assert call() == 0
    for bad in (dict(pairs=None), dict(n=0), dict(out=None), dict(cfg_=None), dict(ch_=None), dict(flags=0)):
        assert call(**bad) == L.AICP_ERR_INVALID, bad
    q, keep2 = L.make_pair(a["ref"], a["read"])
    q.n_read = 0
    assert call(pairs=q) == L.AICP_ERR_INVALID and "pair 0" in ctx.last_error()
