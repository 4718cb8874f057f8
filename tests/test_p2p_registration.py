"""Point-to-point chains (PointToPointErrorMinimizer, knn_normals == 0) through the public calls.

CPU: the parser accepts the 2-D testing chain's text and the bare-minimizer form and still refuses
what it refused; the seeds of the whole-run cases keep the reference's checker margin.
GPU: whole runs on clouds of 2 000 - 4 000 points against p2p_reference.icp_reference (transforms
within 1e-6 rad / 1e-5 m, the parity bar; iteration counts, converged and status equal: the
reference raises MarginError where a smoothed cv0 / cv1 comes within 2e-6 rad / 2e-5 m of its
threshold); register, register_batch and align_batch bit for bit on one pair; one context
alternating minimizers against fresh contexts; the reference cache; the frame-to-reference stream's
refusal; a minimal localization stream against its hand composition.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import localization_reference as lr
import p2p_reference as pr
from aicp_mapping_amd import synthetic as sy

f32 = np.float32
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the parser (CPU) -------
def _parse(L, tmp_path, text, name="c.yaml"):
    p = tmp_path / name
    p.write_text(text)
    return L.parse_pm_yaml(str(p))


def test_parser_accepts_the_2d_testing_chain(L, tmp_path):
    for i, text in enumerate((pr.chain_text(),                                      # "errorMinimizer:\n  Name"
                              pr.chain_text().replace("errorMinimizer:\n  PointToPointErrorMinimizer\n",
                                                      "errorMinimizer: PointToPointErrorMinimizer\n"),
                              pr.chain_text(ref_normals=False))):                   # SurfaceNormal is optional
        rc, c = _parse(L, tmp_path, text, f"c{i}.yaml")
        assert rc == 0, i
        assert c.knn_normals == 0 and c.trimmed_ratio == f32(0.75) and c.max_iter == 100, i
        assert (c.min_diff_rot, c.min_diff_trans, c.smooth_length) == (f32(1e-4), f32(1e-4), 4), i
        assert c.nn_epsilon == 0 and c.knn_match == 1 and c.bucket_size == 8, i


def test_parser_still_refuses_what_it_refused(L, tmp_path):
    un = L.AICP_ERR_UNSUPPORTED
    besl = "  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
    for i, text in enumerate((pr.chain_text(extra_filter=besl),
                              pr.chain_text(extra_filter="  - MinDistDataPointsFilter:\n      minDist: 1.0\n"),
                              pr.chain_text(extra_filter="  - MaxDensityDataPointsFilter:\n      maxDensity: 50\n"),
                              pr.chain_text(minimizer="PointToPlaneWithCovErrorMinimizer"),
                              # the map form of the minimizer: refused before, pinned by test_library_cpu.py
                              pr.chain_text(minimizer="PointToPointErrorMinimizer:"),
                              pr.chain_text(minimizer="PointToPlaneErrorMinimizer:\n    force2D: 1"),
                              pr.chain_text(minimizer="PointToPlaneErrorMinimizer", ref_normals=False),
                              pr.chain_text().replace("TrimmedDistOutlierFilter", "MaxDistOutlierFilter"))):
        assert _parse(L, tmp_path, text, f"u{i}.yaml")[0] == un, i


def test_point_to_plane_chain_parses_as_before(L, tmp_path):
    rc, c = _parse(L, tmp_path, pr.chain_text(minimizer="PointToPlaneErrorMinimizer"))
    assert rc == 0 and c.knn_normals == 10 and c.trimmed_ratio == f32(0.75) and c.max_iter == 100
    d = L.default_config()
    assert (d.knn_normals, d.max_iter, d.smooth_length) == (20, 20, 4)


# ------------------------------------------------------------------ whole runs -------------
def _scene_pair():
    p = sy.make_pair(3000, 3000, seed=7, half=12.0)
    return np.ascontiguousarray(p.ref, f32), np.ascontiguousarray(p.read, f32)


def _cube_pair():
    """The golden cube recipe on a coarser cube (2 400 points): the cube moved by a small yaw and shift.
    Seed 5: with the recipe's seed 3 (and 8, 10) the reference's cv1 / cv0 passes within the margin
    of the threshold and icp_reference raises MarginError."""
    cube = sy.make_cube(step=0.2)
    rng = np.random.default_rng(5)
    T = sy.make_T(yaw_deg=rng.normal(0, 1.0), pitch_deg=0, roll_deg=0, t=(rng.normal(0, 0.1), rng.normal(0, 0.1), 0.0))
    return cube, sy.transform(np.linalg.inv(T), cube).astype(f32)


def _scan_pair():
    """A 2-D scan lifted to z = 0 (2 400 points on three walls): M has rank 2 in every iteration."""
    x = np.linspace(-5, 5, 800)
    rng = np.random.default_rng(5)
    P = np.c_[np.r_[x, x, np.full(800, -5.0)], np.r_[np.full(800, -3.0), np.full(800, 3.0), x * 0.6], np.zeros(2400)]
    P[:, :2] += 0.005 * rng.normal(size=(2400, 2))
    P = P.astype(f32)
    T = sy.make_T(yaw_deg=2.0, pitch_deg=0.0, roll_deg=0.0, t=(0.08, -0.05, 0.0))
    return P, sy.transform(np.linalg.inv(T), P).astype(f32)


CLOUDS = dict(scene=_scene_pair, cube=_cube_pair, scan=_scan_pair)


@functools.lru_cache(maxsize=None)
def whole_run(name):
    """(ref, read, the reference's result): computed once and shared."""
    ref, read = CLOUDS[name]()
    return ref, read, pr.icp_reference(ref, read)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_chosen_seeds_keep_the_margin(oracle, name):
    """icp_reference raises MarginError inside the margin; the runs end by the differential checker
    after more iterations than the smoothing length, well before the counter."""
    ref, read, want = whole_run(name)
    assert 2000 <= len(ref) <= 4000 and 2000 <= len(read) <= 4000
    print(name, "iterations", want["iterations"], "converged", want["converged"], "last cv", want["cv"][-1])
    assert want["status"] == 0 and want["converged"] == 1 and 4 < want["iterations"] < 100


def p2p_cfg(L, tmp_path):
    rc, cfg = _parse(L, tmp_path, pr.chain_text(), "p2p.yaml")
    assert rc == 0
    return cfg


@gpu
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_whole_run_matches_the_reference(ctx, L, oracle, tmp_path, name):
    ref, read, want = whole_run(name)
    T, st = ctx.register(ref, read, p2p_cfg(L, tmp_path))
    r, t = sy.rot_err(want["T"], T)
    print(f"{name}: {st['iterations']} iterations, {r:.2e} rad, {t:.2e} m against the reference")
    assert r <= 1e-6 and t <= 1e-5, (r, t)
    assert (st["status"], st["iterations"], st["converged"]) == (want["status"], want["iterations"], want["converged"])
    assert st["degenerate_normals"] == 0 and st["trimmed_ratio"] == f32(0.75)
    assert st["inlier_ratio"] == f32(np.float64(f32(want["kept"][-1])) / np.float64(len(read)))


@gpu
def test_register_batch_and_align_batch_agree_bit_for_bit(ctx, L, tmp_path):
    ref, read, _ = whole_run("scene")
    cfg = p2p_cfg(L, tmp_path)
    # align_batch with the overlap: the ratio is the auto-tuned one; the other calls are given it
    Ta, sta, rc = ctx.align_batch([dict(ref=ref, read=read)], cfg=cfg, flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP)
    assert rc == 0 and sta[0]["overlap_percent"] > 0
    cfg.trimmed_ratio = sta[0]["trimmed_ratio"]
    T1, st1 = ctx.register(ref, read, cfg)
    others = [whole_run("cube")[1], whole_run("scan")[1]]
    arr = (L.Pair * 3)()
    keep = []
    for i, rd in enumerate([others[0], read, others[1]]):   # three pairs sharing one reference
        arr[i], k = L.make_pair(ref, rd)
        keep.append(k)
    outT = np.zeros((3, 16), f32)
    st = (L.IcpStats * 3)()
    rc = L.lib.aicp_hip_register_batch(ctx.h, C.byref(cfg), arr, 3, L._fptr(outT), st)
    assert st[1].status == 0 and rc in (0, st[0].status, st[2].status)
    Tb = outT[1].reshape(4, 4).T
    assert T1.tobytes() == Tb.tobytes() == Ta[0].tobytes()
    keys = ("iterations", "converged", "inlier_ratio", "trimmed_ratio", "nn_points_touched", "nn_nodes_touched")
    for k in keys:
        assert st1[k] == getattr(st[1], k) == sta[0][k], k
    # the resident batch (aicp_hip_batch_run) and the multi-device call run the same run_batch
    rb = ctx.upload([dict(ref=ref, read=read)])
    assert rb.run(cfg, flags=L.AICP_RUN_ICP) == 0
    Tr, str_ = rb.transforms(), rb.stats_dicts()
    rb.free()
    mc = L.MultiContext(devices=[0])
    Tm, stm, _, rc = mc.align_batch([dict(ref=ref, read=read)], cfg=cfg)
    mc.close()
    assert rc == 0 and T1.tobytes() == Tr[0].tobytes() == Tm[0].tobytes()
    for k in keys:
        assert st1[k] == str_[0][k] == stm[0][k], k


def _both(c, L, ref, read, p2p):
    plane = L.default_config(trimmed_ratio=0.75)
    return [c.register(ref, read, p2p if k else plane) for k in (0, 1, 0, 1, 1, 0)]


@gpu
def test_alternating_minimizers_on_one_context_equal_fresh_contexts(ctx, L, tmp_path):
    """The reference cache keys on knn_normals: a point-to-point call after a point-to-plane call on
    the same reference (and the reverse) rebuilds; no wait sees an event of an earlier call."""
    ref, read, _ = whole_run("scene")
    p2p = p2p_cfg(L, tmp_path)
    plane = L.default_config(trimmed_ratio=0.75)
    c = L.Context(0)
    s0 = c.reference_cache_stats()
    mixed = _both(c, L, ref, read, p2p)
    s1 = c.reference_cache_stats()
    c.close()
    # plane, p2p, plane, p2p build; the second of two consecutive p2p calls hits; the last plane call builds
    assert s1["tree_builds"] - s0["tree_builds"] == 5 and s1["tree_hits"] - s0["tree_hits"] == 1
    fresh = []
    for k in (0, 1):
        f = L.Context(0)
        fresh.append(f.register(ref, read, p2p if k else plane))
        f.close()
    for i, k in enumerate((0, 1, 0, 1, 1, 0)):
        assert mixed[i][0].tobytes() == fresh[k][0].tobytes(), i
        assert mixed[i][1] == fresh[k][1], i
    assert mixed[1][1]["degenerate_normals"] == 0
    assert not np.array_equal(fresh[0][0], fresh[1][0])   # (two different minimizers)


@gpu
def test_second_point_to_point_call_hits_the_cached_tree(L, tmp_path):
    ref, read, _ = whole_run("cube")
    c = L.Context(0)
    cfg = p2p_cfg(L, tmp_path)
    a = c.register(ref, read, cfg)
    s1 = c.reference_cache_stats()
    b = c.register(ref, read, cfg)
    s2 = c.reference_cache_stats()
    c.close()
    assert (s1["tree_builds"], s1["tree_hits"]) == (1, 0) and (s2["tree_builds"], s2["tree_hits"]) == (1, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@gpu
def test_frame_to_reference_stream_refuses_the_chain(ctx, L, tmp_path):
    ref, read, _ = whole_run("cube")
    T, res, done, rc = ctx.sequence_run(ref, (0, 0, 0), [read], [(0, 0, 0)], cfg=p2p_cfg(L, tmp_path),
                                        raise_on_error=False)
    assert rc == L.AICP_ERR_UNSUPPORTED and done == 0
    assert "point-to-point chain in the frame-to-reference stream" in ctx.last_error()
    T, res, done, rc = ctx.sequence_run(ref, (0, 0, 0), [read], [(0, 0, 0)], cfg=p2p_cfg(L, tmp_path),
                                        raise_on_error=False, prefilter=True)
    assert rc == L.AICP_ERR_UNSUPPORTED
    assert "point-to-point chain in the frame-to-reference stream" in ctx.last_error()


@gpu
def test_localization_stream_equals_its_hand_composition(ctx, L, oracle, tmp_path):
    """Two readings on a map of a few thousand points: the stream against register_batch calls
    window by window (merge and re-filter as App's counters ask), bit for bit."""
    from aicp_mapping_amd.prior_map import PriorMap

    mp = np.ascontiguousarray(lr.make_map(oracle)[::12])   # (a map of about 5 000 points)
    reads, poses, _ = lr.make_stream(2, {})
    cfg = L.default_config(point_to_point=True, trimmed_ratio=0.5)
    prm = L.default_localization_params(**lr.PARAMS)
    pm = PriorMap(ctx, mp)
    T, res, done, rc = pm.sequence_run(reads, poses, cfg=cfg, params=prm)
    final = pm.getCloud()
    pm.free()
    assert rc == 0 and done == 2 and all(r["status"] == 0 and r["icp"]["iterations"] > 0 for r in res)
    pm = PriorMap(ctx, mp)
    n_clouds, p, Ts, sts = 0, 0, [], []
    assert prm.flags & L.AICP_LOC_MERGE
    mc = f32(prm.max_correction_magnitude)
    while p < 2:
        w = L.localization_window(n_clouds, prm, 2 - p)
        Tw, st, rcw = pm.register_batch(reads[p:p + w], poses[p:p + w], prm.crop_min, prm.crop_max, cfg=cfg)
        assert rcw == 0
        for i in range(w):
            Ts.append(Tw[i])
            sts.append(st[i])
            if n_clouds != 0 and any(abs(Tw[i][k, 3]) > mc for k in range(3)):
                continue
            n_clouds += 1
            if (n_clouds - 1) % prm.reference_update_frequency == 0:
                pm.merge(reads[p + i], Tw[i])
            if prm.map_refilter_every > 0 and (n_clouds - 1) % prm.map_refilter_every == 0:
                pm.prefilter()
        p += w
    finalc = pm.getCloud()
    pm.free()
    np.testing.assert_array_equal(T, np.stack(Ts))
    assert [r["icp"] for r in res] == sts
    np.testing.assert_array_equal(final, finalc)
    assert 2000 <= len(mp) <= 6000
