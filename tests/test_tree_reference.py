"""tree_reference.py against the C++ oracle, and the conditions its case matrix states (CPU only).

For every case of the matrix that tests/test_tree_kernels.py runs on the device: the plain Python
buildNodes equals pyoracle.Tree's export and info (clouds of up to 20 000 points), the stated
conditions on the data hold (depth range, a sum beyond 2^64, equal extents, a cut at zero), and
the control-block counters expected for the case's plan show the path the case is there for.
"""
import functools

import numpy as np
import pytest

import tree_reference as tr

f32 = np.float32
PY_MAX = 20000  # the Python build runs on clouds up to this size


@functools.lru_cache(maxsize=None)
def _trees(data, center, bucket):
    import pyoracle as po

    out = []
    for p in tr.clouds_of(data):
        pts, _ = tr.centred(p, center)
        out.append((tr.oracle_tree(po, pts, bucket), tr.build_tree(pts, bucket) if len(pts) <= PY_MAX else None))
    return out


@pytest.mark.parametrize("c", tr.CASES + [tr.OVER_LIMIT], ids=lambda c: c.name)
def test_case_reference_oracle_and_conditions(oracle, c):
    clouds, pts, means = tr.case_inputs(c)
    both = _trees(c.data, c.center, c.bucket)
    for i, (want, py) in enumerate(both):
        assert sorted(want["bucket_ids"].tolist()) == list(range(len(pts[i])))
        if py is not None:
            tr.assert_same_tree(py, want, f"{c.name} cloud {i}")
            assert py["leaves"] == want["leaves"]
    trees = [w for w, _ in both]
    # the path the case is there for, from the counters its plan must leave
    needed, n_max = 0, max(len(p) for p in pts)
    for _ in range(c.repeat):
        plan = tr.plan_levels(n_max, needed, c.opts.get("tree_plan", 0))
        ctl = tr.expected_ctl(trees, c.bucket, plan)
        for name in c.path:
            assert tr.PATHS[name](ctl), (c.name, name, plan, ctl)
        if plan:
            needed = tr.needed_after(plan, ctl)
    for cond in c.cond:
        kind = cond if isinstance(cond, str) else cond[0]
        if kind == "depth":
            assert all(cond[1] <= t["tree_depth"] <= cond[2] for t in trees), [t["tree_depth"] for t in trees]
        elif kind == "carry":  # the centroid sum needs the high word on this many axes
            sums = tr.fixed40_sums(clouds[0])
            assert sum(abs(s) >= 2 ** 64 for s in sums) >= cond[1], sums
            assert all(abs(float(m) - clouds[0][:, d].astype(np.float64).mean()) < 1.0 for d, m in enumerate(means[0]))
        elif kind == "equal_extents":
            e = pts[0].max(0) - pts[0].min(0)
            assert e[0] == e[1] == e[2] > 0 and trees[0]["cd"][0] == 0  # the first of equal extents
        elif kind == "zero_cut":
            t = trees[0]
            at0 = np.flatnonzero((t["cd"] != tr.LEAF) & (t["cut"] == 0))
            assert at0.size > 0
            for d in range(3):
                z = pts[0][:, d]
                assert np.any(np.signbit(z) & (z == 0)) and np.any(~np.signbit(z) & (z == 0))
        elif kind == "one_tile":
            assert len(clouds) == 64 and sum(len(p) for p in clouds) <= tr.TILE
            assert all(9 <= len(p) <= 40 for p in clouds)
        else:
            raise AssertionError(cond)


def test_thresholds_are_the_sources():
    """SUB_MAX, MID_MAX, FAR_STACK and the tile restate the build's constants."""
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aicp_mapping_amd", "csrc")
    common = open(os.path.join(csrc, "aicp_common.hpp")).read()
    tree = open(os.path.join(csrc, "kernels_tree.hip")).read()
    assert int(re.search(r"#define AICP_SUBMAX (\d+)", common).group(1)) == tr.SUB_MAX
    assert int(re.search(r"#define AICP_MIDMAX (\d+)", common).group(1)) == tr.MID_MAX
    assert int(re.search(r"constexpr int kFarStack = (\d+)", common).group(1)) == tr.FAR_STACK
    assert "kTile = 256 * kTileItems" in tree and "kTileItems = 8;" in tree and tr.TILE == 2048
    assert "kLbThreads = 256;" in tree and "kLbItems = 8;" in tree


def test_mean_from_fixed40_beyond_one_word():
    """The two-word conversion: exact sums on both sides of 2^64, both signs, against the integer
    quotient's nearest float (one rounding to double of each word, then float)."""
    for acc, n in ((2 ** 64 - 1, 3), (2 ** 64, 3), (2 ** 64 + 12345, 7), (-(2 ** 70) - 99, 10000), (5, 2), (-5, 2),
                   (0, 9)):
        got = tr.mean_from_fixed40(acc, n)
        want = acc / n / 2.0 ** 40  # Python's int / int is correctly rounded
        assert abs(float(got) - want) <= abs(want) * 2.0 ** -23 and (got < 0) == (acc < 0), (acc, n, got, want)
    x = np.array([0.1, -0.25, 3.0], f32)
    assert tr.mean_fixed40(np.stack([x, x, x], 1))[0] == f32(sum(tr.fixed40(x)) / 3 / 2.0 ** 40)


def test_entry_argument_checks():
    """aicp_hip_test_tree refuses bad arguments before any device work."""
    import ctypes as C

    import aicp_mapping_amd._lib as L

    assert "aicp_hip_test_tree" in L.EXPORTS and callable(L.Context.test_tree)
    u32p, ip, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    buf = (C.c_uint32 * 64)()
    fbuf = (C.c_float * 64)()
    a = lambda t: C.cast(buf, t)
    good = [None, 1, a(u32p), C.cast(fbuf, fp), 0, 8, a(u32p), a(u32p), a(ip), C.cast(fbuf, fp), a(u32p),
            C.cast(fbuf, fp), a(u32p)]
    assert L.lib.aicp_hip_test_tree(*good) == L.AICP_ERR_INVALID  # no context
