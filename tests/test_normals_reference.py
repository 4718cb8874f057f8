"""normals_reference.py against the C++ oracle, and the conditions its case matrix states (CPU only).

For every case of the matrix that tests/test_normals_kernels.py runs on the device: the plain
Python recurseKnn gives the oracle's ao_tree_knn lists entry by entry and its touched totals, for
every point of every cloud (auto_rule, 300 001 points, is the oracle's alone); the oracle's
ao_surface_normals passes check_normals under the classes that normal_inputs derives from the
exact covariance (rank <= 1: exactly e_y and counted; regular: norm, Rayleigh excess, sine); and
every condition the case states holds on the reference alone. The figures are printed (DESIGN 4.4
quotes them).
"""
import numpy as np
import pytest

import normals_reference as nr

f32 = np.float32


@pytest.mark.parametrize("c", nr.CASES, ids=lambda c: c.name)
def test_case_reference_oracle_and_conditions(oracle, c):
    pts = nr.clouds(c.make)
    want = nr.oracle_knn(c)
    if c.python:
        for r, (e, w) in enumerate(zip(nr.python_knn(c), want)):
            bad = np.flatnonzero(np.any(e["ids"] != w["ids"], axis=1))
            assert bad.size == 0, (c.name, r, bad[:8].tolist(), e["ids"][bad[:4]].tolist(), w["ids"][bad[:4]].tolist())
            assert (int(e["points"].sum()), int(e["nodes"].sum())) == (w["points"], w["nodes"]), (c.name, r)
    for r, (p, w) in enumerate(zip(pts, want)):  # the lists are lists: ascending, the query first among equals
        d2 = nr.list_d2(p, w["ids"])
        assert np.all(d2[:, 1:] >= d2[:, :-1]) and np.all(d2[:, 0] == 0), (c.name, r)
        assert np.array_equal((w["ids"] >= 0).sum(1), np.full(len(p), min(c.K, len(p)))), (c.name, r)
    figs = []
    for r, (p, ni) in enumerate(zip(pts, nr.inputs(c))):
        nrm, _, deg = oracle.surface_normals(p, c.K)
        figs.append(nr.check_normals(ni, nrm, deg, (c.name, r)))
    tot = {k: (max if k in ("norm", "excess", "sine") else sum)(f[k] for f in figs) for k in figs[0]}
    print(f"{c.name}: oracle normals {tot}")
    for cond in c.cond:
        holds, figure = nr.check_cond(c, cond)
        print(f"{c.name}: {cond} -> {figure}")
        assert holds, (c.name, cond, figure)
    if c.python:
        print(f"{c.name}: nesting {max(int(e['nest'].max()) for e in nr.python_knn(c))}")


def test_every_case_is_listed():
    names = [c.name for c in nr.CASES]
    assert len(set(names)) == len(names)
    for stem, ks in (("tiny", (10, 20, 30)), ("ragged_refs", (20,)), ("scene_dups", (10, 20, 30)), ("scene_dups_far", (20,)),
                     ("lattice", (10, 20, 30)), ("identical", (20,)), ("line", (20,)), ("deep_line", (10, 20, 30)),
                     ("deep_ladder", (10, 20, 30)), ("deep_zigzag", (10, 20, 30)),
                     ("uniform", (10, 20, 30)), ("auto_rule", (10,))):
        for K in ks:
            assert f"{stem}_k{K}" in names
    assert all(n in names for n in nr.CLEAN_CONTEXT)
    for c in nr.CASES:  # both caps hold in every case: stated, or every point is of rank <= 1
        assert {"undecided_cap", "gapless_cap"} <= set(c.cond) or "all_rank1" in c.cond, c.name
    assert max(sum(len(p) for p in nr.clouds(c.make)) for c in nr.CASES if c.python) <= 24240
    assert [c.name for c in nr.CASES if not c.python] == ["auto_rule_k10"]
    # the engine rule is stated by a case on each side of its threshold
    assert nr.by_name("uniform_k10").engine0 == 1 and nr.by_name("auto_rule_k10").engine0 == 2


def test_the_list_is_libnabos_sorted_vector():
    """Equal distances keep their order of arrival; a candidate equal to the head does not enter."""
    import pyoracle as po

    p = np.zeros((12, 3), f32)
    p[8:, 0] = 1  # 8 points at the origin, then 4 at distance 1
    t = po.Tree(p, 16)  # one bucket: arrival order is the bucket's order
    e = nr.knn(t.export(), p, 10)
    order = t.export()["bucket_ids"].tolist()
    zeros, ones = [i for i in order if i < 8], [i for i in order if i >= 8]
    assert e["ids"][0].tolist() == zeros + ones[:2]
    assert e["ids"][11].tolist() == ones + zeros[:6]
    assert np.array_equal(e["ids"], t.knn(p, 10, 0.0, True)[0])


def test_the_climb_time_offset_is_the_entry_time_offset():
    """knn_forgetful (the wrong traversal of the condition frames_matter) reads a node's old offset
    after the near descent, as the device does; with no frame forgetting anything it is knn."""
    c = nr.by_name("deep_zigzag_k20")
    e = nr.python_knn(c)[0]
    n = len(nr.clouds(c.make)[0])
    w = nr.knn_forgetful(nr.oracle_tree(c.make, 0).export(), nr.clouds(c.make)[0], c.K, range(n), 48)
    assert all(np.array_equal(w[k], e[k]) for k in ("ids", "points", "nodes", "nest"))


def test_the_checks_bite():
    """check_normals refuses a normal turned by 2e-7 rad, one scaled by 1 + 2e-7, one that is not
    a number (in one component, in all, at one point, at many), an infinite one, a zero one, a
    rank-1 point whose normal is not e_y bit for bit and a degenerate count off by one."""
    c = nr.by_name("uniform_k10")
    ni = nr.inputs(c)[0]
    good = ni["vec"][:, :, 0].astype(f32)
    assert nr.check_normals(ni, good, 0)["regular"] == 4096
    i = 7
    v = ni["vec"][i, :, 0] + 2e-7 * ni["vec"][i, :, 1]
    nan = f32(np.nan)
    for wrong in ((v / np.linalg.norm(v)), ni["vec"][i, :, 0] * (1 + 2e-7), (nan, nan, nan), (good[i, 0], nan, good[i, 2]),
                  (np.inf, 0, 0), (0, 0, 0)):
        n = good.copy()
        n[i] = np.asarray(wrong).astype(f32)
        assert not np.array_equal(n[i], good[i])
        with pytest.raises(AssertionError):
            nr.check_normals(ni, n, 0)
    n = good.copy()
    n[100:201] = nan
    with pytest.raises(AssertionError):
        nr.check_normals(ni, n, 0)
    with pytest.raises(AssertionError):
        nr.check_normals(ni, good, 1)
    line = nr.inputs(nr.by_name("line_k20"))[0]
    ey = np.tile(np.array([0, 1, 0], f32), (nr.LINE_N, 1))
    assert nr.check_normals(line, ey, nr.LINE_N)["rank1"] == nr.LINE_N
    ey[5, 0] = -0.0  # (equal as a number, not bit for bit)
    with pytest.raises(AssertionError):
        nr.check_normals(line, ey, nr.LINE_N)


def test_constants_are_the_sources():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = lambda *p: open(os.path.join(root, *p)).read()
    icp = src("aicp_mapping_amd", "csrc", "kernels_icp.hip")
    assert int(re.search(r"#define AICP_KNN_LDS_FRAMES (\d+)", icp).group(1)) == nr.LANE_FRAMES
    assert int(re.search(r"kFrames = G == 8 \? (\d+)", icp).group(1)) == nr.OCT_FRAMES
    assert int(re.search(r"constexpr uint32_t kKnnOctMax = (\d+);", icp).group(1)) == nr.OCT_MAX
    assert int(re.search(r"constexpr int kNormalsBucket = (\d+);", src("aicp_mapping_amd", "csrc", "runtime.hpp")).group(1)) \
        == nr.RAW_BUCKET
    assert int(re.search(r"#define AICP_TEST_NN_SENTINEL (0x[0-9A-Fa-f]+)u", src("include", "aicp_hip.h")).group(1), 16) \
        == nr.SENTINEL
    # no search and no normal gives the sentinel: a position beyond 2^28, a NaN
    assert nr.SENTINEL >= 2 ** 28 and np.isnan(np.array([nr.SENTINEL], np.uint32).view(f32)[0])


def test_entry_argument_checks():
    """aicp_hip_test_normals refuses a call without a context before any device work (the other
    conditions: test_normals_kernels.py, with a context)."""
    import ctypes as C

    import aicp_mapping_amd._lib as L

    assert "aicp_hip_test_normals" in L.EXPORTS and callable(L.Context.test_normals)
    u32p, ip, fp, up = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    buf = (C.c_uint32 * 64)(*([1] + [0] * 63))
    fbuf = (C.c_float * 64)()
    i32, f, u64 = C.cast(buf, ip), C.cast(fbuf, fp), C.cast(buf, up)
    good = [None, 1, C.cast(buf, u32p), f, 10, 8, i32, i32, i32, f, i32, u64, f, i32, i32, u64]
    assert L.lib.aicp_hip_test_normals(*good) == L.AICP_ERR_INVALID  # no context
