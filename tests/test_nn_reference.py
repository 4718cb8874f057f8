"""nn_reference.py against the C++ oracle, and the conditions its case matrix states (CPU only).

For every case of the matrix that tests/test_nn_kernels.py runs on the device: the plain Python
recurseKnn equals the oracle's per-query results (ao_tree_nn1: id, d2, touched points and nodes,
nesting of far descents, depth of the deepest far descent's node, largest far bound) on every
query, or on a fixed evenly spaced subset of 96 where the case has more than 300; at epsilon 0
the distance is also the brute-force minimum within the radius. The oracle's per-query form sums
to what its batch form (ao_tree_knn) reports. Every condition a case states holds on the
reference alone, and its figure is printed (DESIGN 4.1 quotes them).
"""
import numpy as np
import pytest

import nn_reference as nr

f32 = np.float32
KEYS = ("id", "d2", "points", "nodes", "nest", "far_depth", "max_bound")


def _subset(c):
    """(step, pair, query) of the queries the Python traversal runs on."""
    inp = nr.inputs(c.make)
    S, P = inp.T.shape[:2]
    every = [(s, p, j) for s in range(S) for p in range(P) if nr.is_active(c, s, p) for j in range(len(inp.reads[p]))]
    if len(every) <= 300:
        return every
    return [every[i] for i in np.linspace(0, len(every) - 1, 96).astype(int)]


@pytest.mark.parametrize("c", [c for c in nr.CASES if c.engine == 0 or c.bucket > 15], ids=lambda c: c.name)
def test_case_reference_oracle_and_conditions(oracle, c):
    inp = nr.inputs(c.make)
    want = nr.expected(c)
    picks = _subset(c)
    assert len(picks) >= min(64, sum(len(r) for r in inp.reads))
    trees = {}
    for s, p in sorted({(s, p) for s, p, _ in picks}):
        r = inp.pair_ref[p]
        if r not in trees:
            trees[r] = nr.oracle_tree(c, r).export()
        js = [j for s2, p2, j in picks if (s2, p2) == (s, p)]
        q = nr.queries(c, s, p)[js]
        got = nr.search(trees[r], inp.refs[r], q, c.eps, c.max_dist)
        for k in KEYS:
            w = want[s][p][k][js]
            same = got[k].view(np.uint32) == w.view(np.uint32) if k in ("d2", "max_bound") else got[k] == w
            assert np.all(same), (c.name, s, p, k, got[k][~same][:4], w[~same][:4])
        assert np.all((got["id"] < 0) == np.isinf(got["d2"]))
        if c.eps == 0:  # exact search: the brute-force minimum within the radius
            d = nr.brute_d2(inp.refs[r], q)
            d = np.where(d <= nr.params(c.eps, c.max_dist)[1], d, f32(np.inf)).min(1)
            assert np.array_equal(d.view(np.uint32), got["d2"].view(np.uint32)), (c.name, s, p)
    for cond in c.cond:
        holds, figure = nr.check_cond(c, cond)
        print(f"{c.name}: {cond} -> {figure}")
        assert holds, (c.name, cond, figure)


@pytest.mark.parametrize("name", ["outside_scratch_eps0", "deep_line_eps316", "lattice", "radius_005_eps316"])
def test_per_query_form_sums_to_the_batch_form(oracle, name):
    """ao_tree_nn1 against ao_tree_knn (k = 1): ids, distances and both touch sums."""
    c = nr.by_name(name)
    for p in range(len(nr.inputs(c.make).reads)):
        q, e = nr.queries(c, 0, p), nr.expected(c)[0][p]
        ids, d2, tp, tn = nr.oracle_tree(c, nr.inputs(c.make).pair_ref[p]).knn(q, 1, c.eps, True, c.max_dist)
        assert np.array_equal(ids[:, 0], e["id"]) and np.array_equal(d2[:, 0].view(np.uint32), e["d2"].view(np.uint32))
        assert (tp, tn) == (int(e["points"].sum(dtype=np.uint64)), int(e["nodes"].sum(dtype=np.uint64)))


def test_transform_order():
    """transform is apply_cols' expression: each row ((T0 x + T1 y) + T2 z) + T3, rounded after
    every operation."""
    rng = np.random.default_rng(3)
    T = rng.normal(size=16).astype(f32)
    p = rng.normal(size=(50, 3)).astype(f32) * f32(100)
    got = nr.transform(T, p)
    for i in range(50):
        for r in range(3):
            o = f32(T[r] * p[i, 0])
            o = f32(o + f32(T[4 + r] * p[i, 1]))
            o = f32(o + f32(T[8 + r] * p[i, 2]))
            o = f32(o + T[12 + r])
            assert o == got[i, r]


def test_touch_word_and_sentinels():
    assert nr.touch_word([3, 70000, 12655], [9, 5, 70000]).tolist() == [3 << 16 | 9, 65535 << 16 | 5, 12655 << 16 | 65535]
    # no search gives the sentinels: a NaN distance, a position beyond 2^28, no inner node with
    # more points than the largest bucket
    assert np.isnan(np.array([nr.SENTINEL], np.uint32).view(f32)[0]) and nr.SENTINEL >= 2 ** 28
    assert nr.TOUCH_SENTINEL >> 16 == 0 and nr.TOUCH_SENTINEL & 0xFFFF > 4096


def test_constants_are_the_sources():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    icp = open(os.path.join(root, "aicp_mapping_amd", "csrc", "kernels_icp.hip")).read()
    hdr = open(os.path.join(root, "include", "aicp_hip.h")).read()
    assert int(re.search(r"#define AICP_NN_LDS_FRAMES (\d+)", icp).group(1)) == nr.LDS_FRAMES
    assert int(re.search(r"constexpr int kPopDepth = (\d+)", icp).group(1)) == nr.POP_DEPTH
    assert "kPmBase = 0x30000000u;  // 2^-31" in icp and np.array([0x30000000], np.uint32).view(f32)[0] == nr.PM_LO
    # code 255 decodes to kPmBase + (254 << 21): 2^32 with mantissa 1.5 -- every bound from there on clamps
    assert np.array([0x30000000 + (254 << 21)], np.uint32).view(f32)[0] == f32(1.5 * nr.PM_HI)
    assert int(re.search(r"#define AICP_TEST_NN_SENTINEL (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == nr.SENTINEL
    assert int(re.search(r"#define AICP_TEST_NN_TOUCH_SENTINEL (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == nr.TOUCH_SENTINEL


def test_entry_argument_checks():
    """aicp_hip_test_nn refuses a call without a context before any device work (the other
    conditions: test_nn_kernels.py, with a context)."""
    import ctypes as C

    import aicp_mapping_amd._lib as L

    assert "aicp_hip_test_nn" in L.EXPORTS and callable(L.Context.test_nn)
    u32p, ip, fp, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    buf = (C.c_uint32 * 64)(*([1] + [0] * 63))
    fbuf = (C.c_float * 64)()
    a = lambda t: C.cast(buf, t)
    dirty = C.c_uint64()
    good = [None, 1, a(u32p), C.cast(fbuf, fp), 8, 1, C.cast((C.c_uint32 * 1)(0), u32p), a(u32p), C.cast(fbuf, fp), 1,
            C.cast(fbuf, fp), None, 0.0, 1.0, a(ip), C.cast(fbuf, fp), a(u32p), a(ip), a(ip), C.byref(dirty)]
    assert L.lib.aicp_hip_test_nn(*good) == L.AICP_ERR_INVALID  # no context
