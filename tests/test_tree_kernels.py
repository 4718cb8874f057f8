"""The production kd-tree build against exact trees, node for node.

Context.test_tree (aicp_hip_test_tree) runs the matcher's batched build (device_trees_begin /
device_trees_end with run_batch's plan, then device_trees_check) on given clouds and downloads what
it wrote. Every case of tree_reference.CASES is compared with the C++ oracle's tree of the same
float32 points (centred with the reference mean for center = 1); test_tree_reference.py holds the
oracle to the plain Python buildNodes on the same cases. All comparisons are equalities: node
counts, depths and offsets, every node's cd, cut (as a float value: a -0.0 / +0.0 cut may differ in
sign, ord_enc orders -0 below +0 and std::min does not), right child or leaf count, bucket start,
parent and depth, the bucket order of the ids, the points bit for bit, the mean bit for bit.

A case cannot pass through another builder: the control block's counters (segments per global
level, n_small, n_mid, n_big) must equal what tree_reference.expected_ctl derives from the exact
trees and the plan, and show the path the case names. Every case builds in a context of its own,
so its plan is the first build's (plan_levels without a previous build).
"""
import functools

import numpy as np
import pytest

import tree_reference as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture()
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def want_trees(data, center, bucket):
    """The oracle's trees of a case's clouds, built once and shared (read-only)."""
    import pyoracle as po

    return tuple(tr.oracle_tree(po, tr.centred(p, center)[0], bucket) for p in tr.clouds_of(data))


def compare(got, c, what):
    """The downloaded build of case c against the oracle; returns nothing, asserts everything."""
    _, pts, means = tr.case_inputs(c)
    want = want_trees(c.data, c.center, c.bucket)
    assert len(got["trees"]) == len(want)
    off = 0
    for i, (g, w) in enumerate(zip(got["trees"], want)):
        tag = f"{what} cloud {i} ({len(pts[i])} points)"
        assert g["node_off"] == off, (tag, g["node_off"], off)  # the running sum of n_nodes
        off += w["n_nodes"]
        t = dict(g, bucket_ids=g["ids"])
        tr.assert_same_tree(t, w, tag)
        assert np.array_equal(g["bpts"].view(np.uint32), pts[i][w["bucket_ids"]].view(np.uint32)), tag
        assert np.array_equal(g["mean"].view(np.uint32), means[i].view(np.uint32)), (tag, g["mean"], means[i])


def run_case(ctx, L, c, rc=0, error=0, builds=None):
    """Build case c (c.repeat times in the same context), compare every build, check the counters
    against the plan each build had. Returns the control blocks."""
    clouds, pts, _ = tr.case_inputs(c)
    want = want_trees(c.data, c.center, c.bucket)
    needed, n_max, ctls = 0, max(len(p) for p in pts), []
    with ctx.options(**c.opts):
        for k in range(builds or c.repeat):
            got = ctx.test_tree(clouds, c.center, c.bucket)
            plan = tr.plan_levels(n_max, needed, c.opts.get("tree_plan", 0))
            ctl, what = got["ctl"], f"{c.name} build {k} plan {plan}"
            print(f"{what}: rc {got['rc']} error {ctl['error']} n_small {ctl['n_small']} n_mid {ctl['n_mid']} "
                  f"n_big {ctl['n_big']} nseg {ctl['nseg'][:int(np.flatnonzero(ctl['nseg']).max()) + 1].tolist()}")
            assert (got["rc"], ctl["error"]) == (rc, error), (what, got["rc"], ctl["error"], got["error"])
            compare(got, c, what)
            exp = tr.expected_ctl(want, c.bucket, plan)
            assert np.array_equal(ctl["nseg"], exp["nseg"]), (what, ctl["nseg"], exp["nseg"])
            assert (ctl["n_small"], ctl["n_mid"], ctl["n_big"]) == (exp["n_small"], exp["n_mid"], exp["n_big"]), \
                (what, ctl, exp)
            for name in c.path:
                assert tr.PATHS[name](ctl), (what, name, ctl)
            if plan:
                needed = tr.needed_after(plan, ctl)
            ctls.append(ctl)
    return ctls


@pytest.mark.parametrize("c", tr.CASES, ids=lambda c: c.name)
def test_build_equals_oracle(ctx, L, c):
    run_case(ctx, L, c)


def test_ragged_clouds_equal_their_own_builds(ctx, L):
    """Each cloud's tree in the ragged batch is the tree of that cloud built alone."""
    c = tr.by_name("ragged")
    clouds, _, _ = tr.case_inputs(c)
    batch = ctx.test_tree(clouds, c.center, c.bucket)
    assert batch["rc"] == 0
    for i, p in enumerate(clouds):
        alone = ctx.test_tree([p], c.center, c.bucket)
        assert alone["rc"] == 0
        a, b = alone["trees"][0], batch["trees"][i]
        assert (a["n_nodes"], a["tree_depth"]) == (b["n_nodes"], b["tree_depth"]), i
        for k in ("cd", "cut_bits", "right_or_count", "bucket_start", "parent", "depth", "ids"):
            assert np.array_equal(a[k], b[k]), (i, k)
        assert np.array_equal(a["bpts"].view(np.uint32), b["bpts"].view(np.uint32)), i
        assert np.array_equal(a["mean"].view(np.uint32), b["mean"].view(np.uint32)), i


def test_second_build_follows_the_first(ctx, L):
    """A context's next plan follows what its last build used: after the shallow first plan of the
    deep ladder the second one is two levels deeper (run_case checks both against the oracle)."""
    c = tr.by_name("deep_ladder_levels")
    first, second = run_case(ctx, L, c)
    assert first["n_big"] > 0 and second["n_big"] > 0
    assert int(np.flatnonzero(second["nseg"]).max()) == int(np.flatnonzero(first["nseg"]).max()) + 2


def test_depth_over_the_limit_is_refused(ctx, L):
    """A tree of 48 levels returns AICP_ERR_UNSUPPORTED (error bit 1) with nothing out of range:
    every builder bounds its stack (subtree_build stops at kFarStack entries, k_tr_mid at kMidStack,
    the block and level builders keep no stack, the host enqueues at most kFarStack - 1 global
    levels) and k_tr_emit reports the depth. The block builder still wrote the whole tree, and the
    context's next build is exact."""
    over = tr.OVER_LIMIT
    clouds, _, _ = tr.case_inputs(over)
    got = ctx.test_tree(clouds, over.center, over.bucket)
    assert got["rc"] == L.AICP_ERR_UNSUPPORTED and got["ctl"]["error"] == tr.ERR_DEPTH, (got["rc"], got["ctl"])
    assert got["trees"][0]["tree_depth"] == tr.FAR_STACK
    compare(got, over, over.name)
    run_case(ctx, L, tr.by_name("deep_line_56"))
    run_case(ctx, L, tr.by_name("size_1025"))


@pytest.mark.parametrize("name", tr.STALLED)
def test_stalled_scan_builds_the_exact_tree(ctx, L, name):
    """The look-back scan's slow path (every tile but the first gives up at once and recomputes its
    exact prefix): the build reports error 16, the call AICP_ERR_HIP, and the tree is the oracle's,
    node for node."""
    c = tr.by_name(name)
    assert L.test_force_scan_stall(True) == L.AICP_OK
    try:
        run_case(ctx, L, c, rc=L.AICP_ERR_HIP, error=tr.ERR_STALL, builds=1)
    finally:
        assert L.test_force_scan_stall(False) == L.AICP_OK
    run_case(ctx, L, c, builds=1)  # and the context's next build is clean


def test_entry_refuses_bad_arguments(ctx, L):
    p = tr.uniform(10, 1)
    import ctypes as C

    u32p, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    counts = np.array([10], np.uint32)
    o = [np.zeros(64, np.uint32) for _ in range(4)] + [np.zeros(64, np.float32) for _ in range(2)]

    def call(n_refs=1, cnt=counts, center=0, bucket=8):
        return L.lib.aicp_hip_test_tree(ctx.h, n_refs, cnt.ctypes.data_as(u32p), L._fptr(p), center, bucket,
                                        o[0].ctypes.data_as(u32p), o[1].ctypes.data_as(u32p), o[2].ctypes.data_as(ip),
                                        L._fptr(o[4]), np.zeros(4 * 22, np.uint32).ctypes.data_as(u32p),
                                        L._fptr(o[5]), o[3].ctypes.data_as(u32p))

    assert call() == L.AICP_OK
    for bad in (dict(n_refs=0), dict(n_refs=4097), dict(cnt=np.array([0], np.uint32)), dict(center=2),
                dict(center=-1), dict(bucket=0), dict(bucket=4097)):
        assert call(**bad) == L.AICP_ERR_INVALID, bad
