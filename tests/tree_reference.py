"""Plain reference of the kd-tree build (kernels_tree.hip) and the case matrix of its tests.

build_tree restates libnabo's KDTreeUnbalancedPtInLeavesImplicitBoundsStackOpt::buildNodes on
float32 values with the sequential two-pass Hoare partition (the device uses the prefix-rank form
of the same partition); mean_fixed40 is the exact order-free centroid. test_tree_reference.py
checks both against the C++ oracle on every case; test_tree_kernels.py compares the device build
(Context.test_tree / aicp_hip_test_tree) with the oracle on the same cases, node for node.

CASES is shared by both test files: what is built (clouds, center, bucket, context options), which
path of the build the case is there for (`path`, a condition on the control block's counters) and
what must hold for its data (`cond`). expected_ctl derives the control block's counters from a
tree and the number of planned global levels, so a case cannot pass by taking another builder.
"""
import collections
import functools
import sys

import numpy as np

f32, f64 = np.float32, np.float64
LEAF = 3
SUB_MAX, MID_MAX = 1024, 8192  # kSubMax, kMidMax (aicp_common.hpp)
TILE = 2048                    # positions per tile of k_tr_sum / k_tr_center / lookback_scan
FAR_STACK = 48                 # kFarStack: trees of depth >= 48 are refused
ERR_DEPTH, ERR_STALL = 1, 16   # TreeCtl::error bits


# ------------------------------------------------------------------ the centroid ------------
def fixed40(col):
    """icp_math.hpp fixed40 per value: round(x * 2^40) as Python ints (saturating at 64 bits)."""
    v = np.rint(np.asarray(col, f32).astype(f64) * 1099511627776.0)
    lim = 9.2233720368547748e18
    return [(2 ** 63 - 1) if not t < lim else (-2 ** 63) if not t > -lim else int(t) for t in v.tolist()]


def mean_from_fixed40(acc, n):
    """icp_math.hpp mean_from_fixed40 on the exact sum `acc` (a Python int of any size): the
    magnitude's two 64-bit words to double one by one, then 2^-40 / n, then float32."""
    mag = -acc if acc < 0 else acc
    hi, lo = mag >> 64, mag & (2 ** 64 - 1)
    m = (float(hi) * 18446744073709551616.0 + float(lo)) * (1.0 / 1099511627776.0) / float(n)
    return f32(-m if acc < 0 else m)


def fixed40_sums(pts):
    return [sum(fixed40(pts[:, d])) for d in range(3)]


def mean_fixed40(pts):
    pts = np.asarray(pts, f32)
    return np.array([mean_from_fixed40(s, len(pts)) for s in fixed40_sums(pts)], f32)


def centred(pts, center):
    """The points the tree is built on, and the mean the build reports (0 without centring)."""
    pts = np.ascontiguousarray(pts, f32)
    if not center:
        return pts, np.zeros(3, f32)
    mean = mean_fixed40(pts)
    return (pts - mean).astype(f32), mean


# ------------------------------------------------------------------ buildNodes --------------
def build_tree(pts, bucket=8):
    """libnabo's buildNodes, recursively, in preorder. Returns the oracle's export (cd, cut,
    right_or_count, bucket_start, bucket_ids) plus n_nodes, tree_depth, leaves, parent, depth."""
    pts = np.ascontiguousarray(pts, f32)
    n = len(pts)
    col = [pts[:, d].astype(f64).tolist() for d in range(3)]  # float32 values, exactly
    idx = list(range(n))
    cd_, cut_, roc_, bs_, ids_ = [], [], [], [], []
    top = [0]
    half = f32(2)

    def build(first, last, mn, mx, depth):
        count = last - first
        pos = len(cd_)
        top[0] = max(top[0], depth)
        if count <= bucket:  # a leaf: its points in their current order
            cd_.append(LEAF)
            cut_.append(0.0)
            roc_.append(count)
            bs_.append(len(ids_))
            ids_.extend(idx[first:last])
            return pos
        cd, best = 0, f32(0)  # the first strict maximum of the box extents, from 0
        for d in range(3):
            e = f32(mx[d]) - f32(mn[d])
            if e > best:
                best, cd = e, d
        ideal = float((f32(mx[cd]) + f32(mn[cd])) / half)
        c = col[cd]
        vals = [c[i] for i in idx[first:last]]
        lo, hi = min(vals), max(vals)
        cut = lo if ideal < lo else (hi if ideal > hi else ideal)
        # pass 1: Hoare partition on (v < cut); pass 2 on (v <= cut) over what is left
        l, r = first, last - 1
        while True:
            while l < last and c[idx[l]] < cut:
                l += 1
            while r >= first and c[idx[r]] >= cut:
                r -= 1
            if l > r:
                break
            idx[l], idx[r] = idx[r], idx[l]
            l += 1
            r -= 1
        br1 = l - first
        r = last - 1
        while True:
            while l < last and c[idx[l]] <= cut:
                l += 1
            while r >= first + br1 and c[idx[r]] > cut:
                r -= 1
            if l > r:
                break
            idx[l], idx[r] = idx[r], idx[l]
            l += 1
            r -= 1
        br2 = l - first
        if ideal < lo:
            left = 1
        elif ideal > hi:
            left = count - 1
        elif br1 > count // 2:
            left = br1
        elif br2 < count // 2:
            left = br2
        else:
            left = count // 2
        cd_.append(cd)
        cut_.append(cut)
        roc_.append(-1)
        bs_.append(-1)
        lmx, rmn = list(mx), list(mn)  # the children's implicit boxes
        lmx[cd] = cut
        rmn[cd] = cut
        build(first, first + left, mn, lmx, depth + 1)
        roc_[pos] = build(first + left, last, rmn, mx, depth + 1)
        return pos

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 1000))
    try:
        build(0, n, [float(v) for v in pts.min(0)], [float(v) for v in pts.max(0)], 0)
    finally:
        sys.setrecursionlimit(old)
    t = dict(cd=np.array(cd_, np.int32), cut=np.array(cut_, f64).astype(f32), right_or_count=np.array(roc_, np.int32),
             bucket_start=np.array(bs_, np.int32), bucket_ids=np.array(ids_, np.int32))
    t.update(n_nodes=len(cd_), tree_depth=top[0], leaves=int((t["cd"] == LEAF).sum()))
    t.update(links(t["cd"], t["right_or_count"]))
    return t


def links(cd, roc):
    """parent, depth and point count of every node from the preorder (left child = node + 1)."""
    n = len(cd)
    parent, depth, count = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for v in range(n):
        if cd[v] != LEAF:
            for c in (v + 1, int(roc[v])):
                parent[c] = v
                depth[c] = depth[v] + 1
    for v in range(n - 1, -1, -1):
        count[v] = roc[v] if cd[v] == LEAF else count[v + 1] + count[roc[v]]
    return dict(parent=parent, depth=depth, count=count)


def oracle_tree(po, pts, bucket):
    """pyoracle.Tree's export and info in build_tree's form."""
    t = po.Tree(pts, bucket)
    ex = t.export()
    n, d, lv = t.info()
    ex.update(n_nodes=n, tree_depth=d, leaves=lv)
    ex.update(links(ex["cd"], ex["right_or_count"]))
    return ex


def assert_same_tree(got, want, what=""):
    """Every field of two trees in build_tree's form, as equalities (the cut as a float value)."""
    assert (got["n_nodes"], got["tree_depth"]) == (want["n_nodes"], want["tree_depth"]), \
        (what, got["n_nodes"], got["tree_depth"], want["n_nodes"], want["tree_depth"])
    for k in ("cd", "right_or_count", "bucket_start", "parent", "depth", "bucket_ids"):
        bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))
        assert got[k].shape == want[k].shape and bad.size == 0, \
            (what, k, bad[:8].tolist(), np.asarray(got[k])[bad[:8]].tolist(), np.asarray(want[k])[bad[:8]].tolist())
    bad = np.flatnonzero(~((got["cut"].view(np.uint32) == want["cut"].view(np.uint32)) |
                           ((got["cut"] == 0) & (want["cut"] == 0))))
    assert bad.size == 0, (what, "cut", bad[:8].tolist(), got["cut"][bad[:8]].tolist(), want["cut"][bad[:8]].tolist())


# ------------------------------------------------------------------ the build's paths -------
def plan_levels(n_max, needed, force):
    """aicp_hip.cpp plan_levels: the global levels a build enqueues (0: the host-polled build)."""
    if force > 0:
        return min(FAR_STACK - 2, force)
    if force < 0:
        return 0
    l = 0
    while (MID_MAX << l) < n_max:
        l += 1
    return min(FAR_STACK - 2, max(l + 1, needed) if needed > 0 else l + 4)


def needed_after(planned, ctl):
    """device_trees_check: what the next plan of the same context follows (polled: unchanged)."""
    used = 0
    while used < FAR_STACK + 1 and ctl["nseg"][used]:
        used += 1
    return min(FAR_STACK - 3, planned + 2) if ctl["n_big"] else used


def expected_ctl(trees, bucket, plan):
    """The control block's counters of a batch of `trees` built with `plan` global levels (0: the
    polled build, as deep as needed). A node above MID_MAX points at a depth below the plan is a
    global-level segment; the first node of at most MID_MAX points on a path goes to the mid-size
    builder, or straight to the subtree builders from SUB_MAX points down; what the mid-size
    builder splits off at <= SUB_MAX goes to the subtree builders; a node still above MID_MAX at the
    plan's depth is an oversized subtree segment (n_big)."""
    nseg = np.zeros(FAR_STACK + 2, np.int64)
    c = collections.Counter()
    nseg[0] = len(trees)
    for t in trees:
        cd, roc, count, depth = t["cd"], t["right_or_count"], t["count"], t["depth"]
        todo = [(0, "global")]
        while todo:
            v, mode = todo.pop()
            n = int(count[v])
            if n <= bucket:
                continue
            if n <= SUB_MAX:
                c["n_small"] += 1
                continue
            if mode == "global":
                if n <= MID_MAX:
                    c["n_mid"] += 1
                    mode = "mid"
                elif plan and depth[v] >= plan:
                    c["n_big"] += 1
                    c["n_small"] += 1
                    continue
                elif depth[v] > 0:
                    nseg[depth[v]] += 1
            todo += [(v + 1, mode), (int(roc[v]), mode)]
    return dict(nseg=nseg, n_small=c["n_small"], n_mid=c["n_mid"], n_big=c["n_big"])


# ------------------------------------------------------------------ data families -----------
def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=f32)


def identical(n):
    return np.tile(np.array([0.3, -1.7, 2.5], f32), (n, 1))


def line(n, seed):
    p = np.zeros((n, 3), f32)
    p[:, 1] = np.random.default_rng(seed).random(n, dtype=f32)
    return p


def plane(n, seed):
    p = uniform(n, seed)
    p[:, 2] = f32(0.5)
    return p


def lattice(n, seed):
    return (np.random.default_rng(seed).integers(0, 8, (n, 3)) * 0.25).astype(f32)


def equal_cube(n, seed):
    p = uniform(n, seed)
    p[0], p[1] = 0, 1  # the three extents are exactly 1
    return p


def signed_zeros(n, seed):
    rng = np.random.default_rng(seed)
    v = np.array([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0, -0.5, 0.5], f32)
    return v[rng.integers(0, len(v), (n, 3))]


def far_away(n, seed):
    c = np.array([4.5e5, 5.1e6, 100.0], f64)
    return (c + np.random.default_rng(seed).uniform(-50, 50, (n, 3))).astype(f32)


def geometric_line(n, seed):
    p = np.zeros((n, 3), f32)
    p[:, 0] = np.ldexp(f32(1), -np.arange(n)).astype(f32)
    return p[np.random.default_rng(seed).permutation(n)]


def ladder(m, rungs, seed):
    rng = np.random.default_rng(seed)
    out = np.full((rungs, 3), 0.5, f32)
    out[:, 0] = np.ldexp(f32(1), np.arange(1, rungs + 1)).astype(f32)
    return np.concatenate([uniform(m, seed + 1), out])[rng.permutation(m + rungs)]


RAGGED = (3, 9, 1000, 1025, 2047, 1, 8193, 8, 4100, 12000)
RAGGED_PERM = (12000, 1, 2047, 8, 8193, 3, 1025, 4100, 9, 1000)


def ragged(counts, seed):
    """clouds of their own sizes, each around its own centre (so that every mean matters)"""
    rng = np.random.default_rng(seed)
    return [(uniform(n, seed + 1 + i) * f32(4) + rng.uniform(-30, 30, 3).astype(f32)).astype(f32)
            for i, n in enumerate(counts)]


def many_small(k, seed):
    rng = np.random.default_rng(seed)
    return ragged([int(n) for n in rng.integers(9, 41, k)], seed + 1)


FAMILIES = dict(uniform=lambda n, seed: [uniform(n, seed)], identical=lambda n: [identical(n)],
                line=lambda n, seed: [line(n, seed)], plane=lambda n, seed: [plane(n, seed)],
                lattice=lambda n, seed: [lattice(n, seed)], equal_cube=lambda n, seed: [equal_cube(n, seed)],
                signed_zeros=lambda n, seed: [signed_zeros(n, seed)], far_away=lambda n, seed: [far_away(n, seed)],
                geometric_line=lambda n, seed: [geometric_line(n, seed)],
                ladder=lambda m, rungs, seed: [ladder(m, rungs, seed)], ragged=ragged, many_small=many_small,
                two=lambda n, seed: [uniform(n, seed), uniform(n, seed + 1)])


@functools.lru_cache(maxsize=None)
def clouds_of(data):
    """The clouds of a case's `data` key (family, arguments...); read-only, shared by the tests."""
    out = FAMILIES[data[0]](*data[1:])
    for c in out:
        c.setflags(write=False)
    return tuple(out)


# ------------------------------------------------------------------ the case matrix ---------
# path: conditions on the control block that say the intended path ran, by name (PATHS below).
# cond: conditions on the data and its exact trees (CPU test), by name: ("depth", lo, hi),
# ("carry", axes), "equal_extents", "zero_cut".
Case = collections.namedtuple("Case", "name data center bucket opts path cond repeat")


def case(name, data, center=0, bucket=8, opts=None, path=(), cond=(), repeat=1):
    return Case(name, tuple(data), center, bucket, dict(opts or {}), tuple(path), tuple(cond), repeat)


PATHS = {
    "root_leaf": lambda c: c["n_small"] == 0 and c["n_mid"] == 0 and c["nseg"][1] == 0,   # k_tr_roots' leaf
    "root_sub": lambda c: c["n_small"] == 1 and c["n_mid"] == 0 and c["nseg"][1] == 0,    # root to the subtree builders
    "root_mid": lambda c: c["n_mid"] == 1 and c["n_small"] >= 2 and c["nseg"][1] == 0,    # root to k_tr_mid
    "level0": lambda c: c["n_mid"] >= 2 and c["n_big"] == 0,                              # root split by a global level
    "levels": lambda c: c["nseg"][1] > 0 and c["n_mid"] > 0 and c["n_big"] == 0,          # two or more global levels
    "mid": lambda c: c["n_mid"] > 0,
    "small": lambda c: c["n_small"] > 0,
    "big": lambda c: c["n_big"] > 0,
    "no_big": lambda c: c["n_big"] == 0,
    "deep_levels": lambda c: c["nseg"][20] > 0,                                           # a long run of global levels
}

U = 11  # seed of the uniform cube


def _cases():
    out = []
    # sizes at bucket 8: leaf from k_tr_roots; subtree root; mid root; global levels
    for n, path in ((1, "root_leaf"), (2, "root_leaf"), (8, "root_leaf"), (9, "root_sub"), (17, "root_sub"),
                    (1024, "root_sub"), (1025, "root_mid"), (8192, "root_mid"), (8193, "level0"), (20000, "levels")):
        out.append(case(f"size_{n}", ("uniform", n, U), path=(path,)))
    # buckets: 1 and 3 every segment through k_tr_subtree, 4 k_tr_subtree_blk at its level cap
    for b in (1, 3, 4, 6, 16):
        out.append(case(f"bucket_{b}_n1024", ("uniform", 1024, U), bucket=b, path=("root_sub",)))
        out.append(case(f"bucket_{b}_n8193", ("uniform", 8193, U), bucket=b, path=("level0", "small")))
    # k_tr_subtree_lvl for every build
    for b in (8, 16):
        out.append(case(f"lvl_builder_b{b}", ("uniform", 8193, U), bucket=b, opts=dict(tree_lvl_min=1),
                        path=("level0", "small")))
    # plans at 20000 points: planned from the size (size_20000), one and two levels (too shallow:
    # oversized segments finished by k_tr_subtree in global memory), host-polled
    out.append(case("plan_1", ("uniform", 20000, U), opts=dict(tree_plan=1), path=("big",)))
    # (two levels are just enough at 20000 points: the last planned level cuts the two halves of
    # 10000 into mid-size segments, so nothing is oversized; at 40000 its children still are)
    out.append(case("plan_2", ("uniform", 20000, U), opts=dict(tree_plan=2), path=("levels", "no_big")))
    out.append(case("plan_2_n40000", ("uniform", 40000, U), opts=dict(tree_plan=2), path=("big",)))
    out.append(case("plan_polled", ("uniform", 20000, U), opts=dict(tree_plan=-1), path=("levels",)))
    # ragged batches: cloud boundaries inside tiles and waves, three clouds in one tile
    out.append(case("ragged", ("ragged", RAGGED, 21), center=1, path=("level0", "small")))
    out.append(case("ragged_perm", ("ragged", RAGGED_PERM, 22), center=1, path=("level0", "small")))
    out.append(case("many_small", ("many_small", 64, 23), center=1, path=("small",), cond=("one_tile",)))
    # degenerate data
    out.append(case("identical", ("identical", 3000), path=("root_mid",)))
    out.append(case("line", ("line", 3000, 31), path=("root_mid",)))
    out.append(case("plane", ("plane", 3000, 32), path=("root_mid",)))
    out.append(case("lattice_b8", ("lattice", 5000, 33), path=("root_mid",)))
    out.append(case("lattice_b1", ("lattice", 5000, 33), bucket=1, path=("root_mid",)))
    out.append(case("equal_cube", ("equal_cube", 3000, 34), path=("root_mid",), cond=("equal_extents",)))
    out.append(case("signed_zeros", ("signed_zeros", 4000, 35), path=("root_mid",), cond=("zero_cut",)))
    # sums beyond one 64-bit word
    out.append(case("far_away", ("far_away", 10000, 36), center=1, path=("level0",), cond=(("carry", 2),)))
    # deep trees: the deepest legal one in a subtree builder, in k_tr_mid, and in the global levels
    # (the second build of the same context follows what the first one used)
    out.append(case("deep_line_56", ("geometric_line", 56, 41), path=("root_sub",), cond=(("depth", 47, 47),)))
    out.append(case("deep_ladder_mid", ("ladder", 1960, 32, 42), path=("root_mid",), cond=(("depth", 40, 47),)))
    out.append(case("deep_ladder_levels", ("ladder", 9000, 32, 43), path=("big",), cond=(("depth", 40, 47),),
                    repeat=2))
    out.append(case("deep_ladder_polled", ("ladder", 9000, 32, 43), opts=dict(tree_plan=-1),
                    path=("deep_levels", "no_big"), cond=(("depth", 40, 47),)))
    # more than 64 scan tiles: the look-back goes round its window
    out.append(case("long_lookback", ("two", 70000, 51), path=("levels",)))
    # ties (the second Hoare pass, on v == cut) where only k_tr_mid and the block builder met them:
    # the level builder's any_eq pass, the wave builder in place in global memory (32-bit
    # positions) and the global levels' pass-2 partner search (k_tr_move2)
    out.append(case("lvl_builder_lattice", ("lattice", 5000, 33), opts=dict(tree_lvl_min=1), path=("root_mid",),
                    cond=(("depth", 16, 16),)))
    out.append(case("lvl_builder_identical", ("identical", 3000), opts=dict(tree_lvl_min=1), path=("root_mid",),
                    cond=(("depth", 9, 9),)))
    out.append(case("plan_1_lattice", ("lattice", 20000, 33), opts=dict(tree_plan=1), path=("big",)))
    out.append(case("levels_lattice", ("lattice", 20000, 33), path=("levels",), cond=(("depth", 18, 18),)))
    return out


CASES = _cases()
# the depth limit: one level too many must be refused, cleanly
OVER_LIMIT = case("deep_line_57", ("geometric_line", 57, 41), path=("root_sub",), cond=(("depth", 48, 48),))


# the scan's slow path (aicp_hip_test_force_scan_stall) on these cases' data
STALLED = ("size_20000", "ragged", "long_lookback")


def by_name(name):
    return next(c for c in CASES + [OVER_LIMIT] if c.name == name)


def case_inputs(c):
    """(clouds as given, the points each tree is built on, the expected means) of a case."""
    clouds = clouds_of(c.data)
    cm = [centred(p, c.center) for p in clouds]
    return clouds, [a for a, _ in cm], [m for _, m in cm]
