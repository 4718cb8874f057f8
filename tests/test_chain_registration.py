"""Whole registrations on sampled chains (aicp_hip_register_chain).

CPU: the seeds of the whole-run cases keep the reference loop's margins, and the MaxDist case's
limit keeps between a quarter and three quarters of the reading in the first iteration.
GPU: an empty chain gives aicp_hip_register's bits; a Besl92-shaped point-to-point chain equals
aicp_hip_register on the two downloaded filtered clouds bit for bit; the icp_3D_cfg_trimmed and
icp_3D_cfg_max shapes against chain_reference.plane_icp_reference at the bar test_p2p_registration.py
holds whole runs to (1e-6 rad, 1e-5 m, equal iteration counts, status, converged and last kept
count); the two convergence errors; HipRegistration on the Besl92 chain file.
"""
import functools
import os

import numpy as np
import pytest

import chain_reference as cr
from aicp_mapping_amd import synthetic as sy

f32 = np.float32
gpu = pytest.mark.gpu
CHAINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chains")


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
def nocache(L):
    """A context whose one-shot calls keep no reference (aicp_hip_options::reference_cache = 0)."""
    c = L.Context(0)
    c.set_options(reference_cache=0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def scene_pair():
    p = sy.make_pair(3000, 3000, seed=7, half=12.0)
    return np.ascontiguousarray(p.ref, f32), np.ascontiguousarray(p.read, f32)


# The icp_3D files' lists. maxDensity 3.75 is about the median density of the 3 000-point reading
# (3.744; the files' 50 would keep every point of so sparse a cloud).
REF_3D = (dict(kind=cr.SN, knn=10, keep_densities=0), dict(kind=cr.RANDOM, prob=0.5))
READ_3D = (dict(kind=cr.SN, knn=10, keep_densities=1), dict(kind=cr.MAX_DENSITY, max_density=3.75))
# name -> (chain seed, MaxDist limit on d2 or None). Seeds chosen on the CPU with the loop alone:
# trimmed: seed 1 is the first tried. max: the limit 0.15 m^2 is about the median first-iteration d2
# (the files' 0.05 keeps 18 % of this pair's first iteration); seeds 1 - 12 put a reading within
# 4e-5 m of the limit in some iteration (MarginError), 13 does not.
WHOLE = dict(trimmed=(1, None), max=(13, 0.15))


def _oracle_densities(oracle, read):
    return oracle.surface_normals(read, 10)[1]


@functools.lru_cache(maxsize=None)
def _cpu_run(name):
    import pyoracle as po

    ref, read = scene_pair()
    seed, lim = WHOLE[name]
    return cr.plane_icp_reference(ref, read, REF_3D, READ_3D, seed, dens_read=_oracle_densities(po, read), limit_d2=lim)


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_chosen_seeds_keep_the_margin(oracle, name):
    want = _cpu_run(name)
    print(name, "iterations", want["iterations"], "kept", want["kept"], "of", want["n_read"], "reference", want["n_ref"])
    assert want["status"] == 0 and want["converged"] == 1 and 4 < want["iterations"] < 100
    assert 1000 < want["n_ref"] < 2000 and 1500 < want["n_read"] < 3000
    if name == "max":
        assert 0.25 < want["kept"][0] / want["n_read"] < 0.75


def plane_cfg(L):
    """The icp_3D files' aicp_icp_config values."""
    return L.default_config(knn_normals=10, nn_epsilon=0.0, trimmed_ratio=0.75, max_iter=100, min_diff_rot=0.001,
                            min_diff_trans=0.001, smooth_length=4)


def p2p_cfg(L):
    """Besl92's: point-to-point, epsilon 3.16, ratio 0.75, 150 iterations, 0.001 / 0.01 / 4."""
    return L.default_config(point_to_point=True, nn_epsilon=3.16, trimmed_ratio=0.75, max_iter=150, min_diff_rot=0.001,
                            min_diff_trans=0.01, smooth_length=4)


# ------------------------------------------------------------------ 1: the empty chain ------
@gpu
@pytest.mark.parametrize("minimizer", ["plane", "point"])
def test_empty_chain_gives_the_bits_of_register(ctx, nocache, L, minimizer):
    ref, read = scene_pair()
    cfg = plane_cfg(L) if minimizer == "plane" else p2p_cfg(L)
    T0, st0 = nocache.register(ref, read, cfg)
    T1, st1, cs, rc = ctx.register_chain(ref, read, cfg, L.Chain())
    assert rc == 0 and T0.tobytes() == T1.tobytes()
    assert st0 == st1 and st0["iterations"] > 0
    assert cs["n_in"] == cs["n_kept"] == [3000, 3000]
    # and a SurfaceNormal-only chain, as the parser gives for the files aicp_hip_parse_pm_yaml accepts
    sn = cr.make_chain(L, [dict(kind=cr.SN, knn=10)], [dict(kind=cr.SN, knn=10, keep_densities=1)])
    T2, st2, _, _ = ctx.register_chain(ref, read, cfg, sn)
    assert T2.tobytes() == T0.tobytes() and st2 == st0


# ------------------------------------------------------------------ 2: Besl92's shape -------
BESL = (dict(kind=cr.MIN_DIST, dim=-1, min_dist=1.0), dict(kind=cr.RANDOM, prob=0.5))


@gpu
def test_besl92_shape_equals_register_on_the_filtered_clouds(ctx, nocache, L):
    ref, read = scene_pair()
    cfg = p2p_cfg(L)
    ch = cr.make_chain(L, BESL, BESL, seed=4)
    T, st, cs, rc = ctx.register_chain(ref, read, cfg, ch)
    fr = ctx.chain_filter(ch, cr.REFERENCE, ref)
    fd = ctx.chain_filter(ch, cr.READING, read)
    assert cs["n_kept"] == [fr["n"], fd["n"]] and cs["n_out"][0][:2] == fr["counts"] and cs["n_out"][1][:2] == fd["counts"]
    assert 1000 < fr["n"] < 2000 and 1000 < fd["n"] < 2000
    # the reference's filters give the same lists
    assert np.array_equal(fr["index"], cr.run_filters(ref, BESL, cr.REFERENCE, 4)["index"])
    assert np.array_equal(fd["index"], cr.run_filters(read, BESL, cr.READING, 4)["index"])
    T2, st2 = nocache.register(ref[fr["index"]], read[fd["index"]], cfg)
    assert rc == 0 and T.tobytes() == T2.tobytes()
    assert st == st2 and st["iterations"] > 0
    # the same seed gives the same sample on every call; another seed another sample
    T3, st3, _, _ = ctx.register_chain(ref, read, cfg, ch)
    assert T3.tobytes() == T.tobytes() and st3 == st
    ch.seed = 5
    assert ctx.chain_filter(ch, cr.READING, read)["index"].tolist() != fd["index"].tolist()


# ------------------------------------------------------------------ 3: the icp_3D shapes -----
@gpu
@pytest.mark.parametrize("name", sorted(WHOLE))
def test_icp_3d_shapes_match_the_reference_loop(ctx, L, oracle, name):
    """Of the kept counts per iteration the C-ABI shows the last one only (inlier_ratio), as in
    test_p2p_registration.py; it and the iteration count are compared. Under MaxDist the loop raises
    MarginError where a reading comes within 4e-5 m of the limit in any iteration, so with the chosen
    seed every iteration's kept set is the same on both sides as long as the transforms stay within
    the bar; the earlier iterations' counts themselves are not read from the device."""
    ref, read = scene_pair()
    seed, lim = WHOLE[name]
    ch = cr.make_chain(L, REF_3D, READ_3D, seed=seed, max_dist_d2=lim)
    T, st, cs, rc = ctx.register_chain(ref, read, plane_cfg(L), ch)
    assert rc == 0
    # the loop takes the device's densities
    dens = ctx.chain_filter(ch, cr.READING, read, densities=True)["densities"]
    want = cr.plane_icp_reference(ref, read, REF_3D, READ_3D, seed, dens_read=dens, limit_d2=lim)
    r, t = sy.rot_err(want["T"], T)
    print(f"{name}: {st['iterations']} iterations, {cs['n_kept']} points, {r:.2e} rad, {t:.2e} m against the reference")
    assert cs["n_kept"] == [want["n_ref"], want["n_read"]]
    assert r <= 1e-6 and t <= 1e-5, (r, t)
    assert (st["status"], st["iterations"], st["converged"]) == (want["status"], want["iterations"], want["converged"])
    assert st["inlier_ratio"] == f32(np.float64(f32(want["kept"][-1])) / np.float64(want["n_read"]))
    assert cs["n_out"][0][:2] == [3000, want["n_ref"]] and cs["n_out"][1][:2] == [3000, want["n_read"]]


# ------------------------------------------------------------------ 4: the two errors -------
@gpu
def test_max_dist_below_every_distance_ends_the_pair(ctx, L):
    ref, read = scene_pair()
    ch = cr.make_chain(L, (), (), max_dist_d2=1e-12)
    T, st, cs, rc = ctx.register_chain(ref, read, plane_cfg(L), ch, raise_on_error=False)
    assert rc == L.AICP_ERR_CONVERGENCE and st["status"] == L.AICP_ERR_CONVERGENCE
    # "no point to minimize" in the first iteration: one NN search ran, no update counted
    assert st["iterations"] == 0 and st["nn_points_touched"] > 0


@gpu
def test_a_side_left_without_points_is_a_convergence_error(ctx, L):
    ref, read = scene_pair()
    far = dict(kind=cr.MIN_DIST, dim=-1, min_dist=1000.0)
    T, st, cs, rc = ctx.register_chain(ref, read, p2p_cfg(L), cr.make_chain(L, (), [far]), raise_on_error=False)
    assert rc == L.AICP_ERR_CONVERGENCE and "reading" in ctx.last_error() and cs["n_kept"] == [3000, 0]
    T, st, cs, rc = ctx.register_chain(ref, read, p2p_cfg(L), cr.make_chain(L, [far], ()), raise_on_error=False)
    assert rc == L.AICP_ERR_CONVERGENCE and "reference" in ctx.last_error() and cs["n_kept"] == [0, 3000]
    with pytest.raises(L.ConvergenceError):
        ctx.register_chain(ref, read, p2p_cfg(L), cr.make_chain(L, [far], ()))


# ------------------------------------------------------------------ 5: the drop-in class ----
@gpu
def test_hip_registration_serves_the_besl92_file(ctx, L, capsys):
    from aicp_mapping_amd import registration as reg

    ref, read = scene_pair()
    path = os.path.join(CHAINS, "Besl92_pt2point.yaml")
    params = reg.RegistrationParams(type="Pointmatcher")
    params.pointmatcher.configFileName = path
    r = reg.create_registrator(params, ctx)
    T = r.registerClouds(ref, read)
    rc, cfg, ch = L.parse_pm_chain(path)
    assert rc == 0 and r.chain_seed == 0
    T2, st2, cs2, _ = ctx.register_chain(ref, read, cfg, ch)
    assert np.asarray(T).tobytes() == T2.tobytes() and r.stats == st2 and r.chain_stats == cs2
    assert cs2["n_kept"][0] < 300 and cs2["n_kept"][1] < 300   # prob 0.05
    r.chain_seed = 3
    assert np.asarray(r.registerClouds(ref, read)).tobytes() != T2.tobytes()
