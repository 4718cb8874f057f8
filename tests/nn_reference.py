"""Plain reference of the ICP loop's NN search (k_icp_nn, kernels_icp.hip) and the case matrix of
its tests.

search restates libnabo's KDTreeUnbalancedPtInLeavesImplicitBoundsStackOpt::recurseKnn (k = 1,
allowSelfMatch) on pyoracle.Tree.export(), in float32 arithmetic in libnabo's order, with the
counters the device reports (touched bucket points, touched inner nodes) and the ones that say
which part of the kernel a query reaches: the deepest nesting of far descents (the kernel keeps
LDS_FRAMES frames in LDS, deeper ones in scratch), the greatest depth of a node whose far child
was entered (frames from depth POP_DEPTH on climb without the pop check) and the largest far
bound (the pop check's one-byte code is 0 below 2^-31 and clamps from 2^32 on).
test_nn_reference.py holds it to the C++ oracle's ao_tree_nn1 on every case; test_nn_kernels.py
compares the device (Context.test_nn / aicp_hip_test_nn) with the oracle, query by query.

CASES is shared by both test files: what is searched (references, bucket, pairs, per-step
transforms and active flags, epsilon, max_dist, context options), the engine the case must run on
and the conditions that must hold on the reference alone (`cond`, COND below).
"""
import collections
import functools
import sys

import numpy as np

import tree_reference as tr

f32 = np.float32
LEAF = tr.LEAF
LDS_FRAMES = 3   # AICP_NN_LDS_FRAMES: far frames per lane kept in LDS
POP_DEPTH = 16   # kPopDepth: depths whose prefix minimum the pop check keeps
PM_LO, PM_HI = 2.0 ** -31, 2.0 ** 32  # the one-byte bound: code 0 below, code 255 from here on
SAT = 65535      # each half of the touch word saturates here
SENTINEL, TOUCH_SENTINEL = 0x7FF8DEAD, 0x0000DEAD  # AICP_TEST_NN_SENTINEL, AICP_TEST_NN_TOUCH_SENTINEL
INF = float("inf")


# ------------------------------------------------------------------ the query ---------------
def transform(T, pts):
    """apply_cols: ((T0 x + T1 y) + T2 z) + T3 per row in float32; T column-major, 16 floats."""
    T = np.asarray(T, f32).reshape(4, 4)  # T[c] = column c
    p = np.ascontiguousarray(pts, f32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    o = T[0, :3] * x
    o = o + T[1, :3] * y
    o = o + T[2, :3] * z
    o = o + T[3, :3]
    return np.ascontiguousarray(o, f32)


def touch_word(nodes, points):
    return (np.minimum(np.asarray(nodes, np.int64), SAT) << 16 | np.minimum(np.asarray(points, np.int64), SAT)) \
        .astype(np.uint32)


def params(eps, max_dist):
    """icp_params: (1 + eps)^2 and max_dist^2 in float32."""
    e = f32(1) + f32(eps)
    with np.errstate(over="ignore"):
        return f32(e * e), f32(f32(max_dist) * f32(max_dist))


# ------------------------------------------------------------------ recurseKnn --------------
def search(tree, pts, queries, eps=0.0, max_dist=INF):
    """The 1-NN of every query in `tree` (Tree.export() of `pts`). Returns dict(id, d2, points,
    nodes, nest, far_depth, max_bound), one entry per query each; id -1 and d2 +inf for none."""
    cd, cut = tree["cd"].tolist(), tree["cut"]
    roc, bs, bid = tree["right_or_count"].tolist(), tree["bucket_start"].tolist(), tree["bucket_ids"].tolist()
    P = np.ascontiguousarray(pts, f32)
    maxE2, maxR2 = params(eps, max_dist)
    zero = f32(0)
    out = collections.defaultdict(list)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        for q in np.ascontiguousarray(queries, f32):
            best = [f32(INF), -1]
            off = [zero, zero, zero]
            c = dict(points=0, nodes=0, nest=0, max_nest=0, far_depth=-1, max_bound=zero)

            def far(rd, depth):
                if rd > c["max_bound"]:
                    c["max_bound"] = rd
                if not (rd <= maxR2 and f32(rd * maxE2) < best[0]):
                    return False
                c["nest"] += 1
                c["max_nest"] = max(c["max_nest"], c["nest"])
                c["far_depth"] = max(c["far_depth"], depth)
                return True

            def recurse(n, rd, depth):
                d = cd[n]
                if d == LEAF:
                    for i in range(bs[n], bs[n] + roc[n]):
                        p = P[bid[i]]
                        dist = zero
                        for k in range(3):
                            diff = f32(q[k] - p[k])
                            dist = f32(dist + f32(diff * diff))
                        if dist <= maxR2 and dist < best[0]:
                            best[0], best[1] = dist, bid[i]
                    c["points"] += roc[n]
                    return
                c["nodes"] += 1
                old_off = off[d]
                new_off = f32(q[d] - cut[n])
                near, other = (roc[n], n + 1) if new_off > 0 else (n + 1, roc[n])
                recurse(near, rd, depth + 1)
                rd = f32(rd + f32(f32(-old_off * old_off) + f32(new_off * new_off)))
                if far(rd, depth):
                    off[d] = new_off
                    recurse(other, rd, depth + 1)
                    off[d] = old_off
                    c["nest"] -= 1

            recurse(0, zero, 0)
            out["id"].append(best[1])
            out["d2"].append(best[0])
            for k, name in (("points", "points"), ("nodes", "nodes"), ("max_nest", "nest"), ("far_depth", "far_depth"),
                            ("max_bound", "max_bound")):
                out[name].append(c[k])
    finally:
        sys.setrecursionlimit(old)
    kinds = dict(id=np.int32, d2=f32, points=np.uint32, nodes=np.uint32, nest=np.int32, far_depth=np.int32,
                 max_bound=f32)
    return {k: np.array(out[k], t) for k, t in kinds.items()}


def brute_d2(pts, queries):
    """Every squared distance in the search's float32 order, (queries, points)."""
    P, Q = np.ascontiguousarray(pts, f32), np.ascontiguousarray(queries, f32)
    d = Q[:, None, :] - P[None, :, :]
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------ queries -----------------
def inside(n, seed, width=1.0):
    return (np.random.default_rng(seed).random((n, 3), dtype=f32) * f32(width)).astype(f32)


def outside(n, seed):
    """in [-2.5, 3.5]^3: up to 2.5 widths outside a unit cloud"""
    return (np.random.default_rng(seed).random((n, 3), dtype=f32) * f32(6) - f32(2.5)).astype(f32)


def line_queries(n):
    """beside the geometric line's points: x = 1.5 * 2^-i, a 1e-6 offset in y"""
    q = np.zeros((n, 3), f32)
    q[:, 0] = (f32(1.5) * np.ldexp(f32(1), -(np.arange(n) % 56))).astype(f32)
    q[:, 1] = f32(1e-6)
    return q


def rigid(seed, angle=0.3, shift=0.2):
    """a rotation about a random axis and a translation, column-major float32[16]"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = angle * rng.uniform(0.5, 1.0)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = rng.uniform(-shift, shift, 3)
    return np.ascontiguousarray(M.T.reshape(16), f32)


IDENT = np.ascontiguousarray(np.eye(4).reshape(16), f32)


# ------------------------------------------------------------------ the case matrix ---------
# refs: tree_reference data keys, one cloud each; scale: a power of two on clouds and readings;
# reads: per pair (reference, readings); T (steps, pairs, 16); active (steps, pairs) or None.
Inputs = collections.namedtuple("Inputs", "refs pair_ref reads T active")
Case = collections.namedtuple("Case", "name make bucket eps max_dist opts engine cond")

UNI = ("uniform", 4096, tr.U)
RAGGED_READS = (1, 63, 64, 65, 130, 7)


def _cloud(key, scale=1.0):
    c = (tr.clouds_of(key)[0] * f32(scale)).astype(f32)
    c.setflags(write=False)
    return c


def _one_step(refs, pairs):
    T = np.tile(IDENT, (1, len(pairs), 1))
    return Inputs(tuple(refs), tuple(r for r, _ in pairs), tuple(q for _, q in pairs), T, None)


def make_inside():
    c = _cloud(UNI)
    return _one_step([c], [(0, inside(600, 5)), (0, c)])


def make_outside(scale=1.0):
    return _one_step([_cloud(UNI, scale)], [(0, (outside(300, 6) * f32(scale)).astype(f32))])


def make_deep_line():
    return _one_step([_cloud(("geometric_line", 56, 41))], [(0, line_queries(200))])


def make_deep_ladder():
    c = _cloud(("ladder", 1960, 32, 42))
    return _one_step([c], [(0, inside(200, 7)), (0, (c[:200] + f32(0.01)).astype(f32))])


def make_identical():
    c = _cloud(("identical", 3000))
    off = (c[:32] + np.random.default_rng(8).uniform(-2, 2, (32, 3)).astype(f32)).astype(f32)
    return _one_step([c], [(0, np.concatenate([c[:32], off]))])


def make_lattice():
    c = _cloud(("lattice", 5000, 33))
    return _one_step([c], [(0, c[:600]), (0, inside(300, 9, 1.75))])


def make_radius():
    return _one_step([_cloud(UNI)], [(0, inside(600, 5)), (0, outside(300, 6))])


def make_buckets():
    return _one_step([_cloud(UNI)], [(0, inside(300, 10)), (0, outside(150, 11))])


def make_saturate():
    c = _cloud(("identical", 70000))
    return _one_step([c], [(0, np.stack([c[0], np.ones(3, f32)]))])


def make_transforms():
    c = _cloud(UNI)
    reads = [(0, inside(300, 12 + p)) for p in range(3)]
    T = np.stack([np.stack([rigid(100 + 10 * s + p) for p in range(3)]) for s in range(3)])
    return Inputs((c,), (0, 0, 0), tuple(q for _, q in reads), T, None)


def make_ragged_pairs():
    refs = [_cloud(("uniform", n, 60 + i)) for i, n in enumerate((1000, 2000, 3000))]
    P = 600
    pair_ref = tuple(p % 3 for p in range(P))
    reads = tuple((inside(RAGGED_READS[p % 6], 1000 + p, 1.4) - f32(0.2)).astype(f32) for p in range(P))
    T = np.stack([np.tile(t, (P, 1)) for t in (IDENT, rigid(200, 0.1, 0.05), IDENT)])
    active = np.ones((3, P), np.uint8)
    active[0, ::5] = 0
    active[1, ::3] = 0
    return Inputs(tuple(refs), pair_ref, reads, T, active)


def make_tiny(shape):
    pairs, n = shape
    return _one_step([_cloud(UNI)], [(0, inside(n, 20 + p)) for p in range(pairs)])


def make_all_inactive():
    inp = _one_step([_cloud(UNI)], [(0, inside(70, 30)), (0, inside(5, 31)), (0, inside(64, 32))])
    active = np.array([[1, 1, 1], [0, 0, 0], [0, 1, 0]], np.uint8)
    return inp._replace(T=np.tile(IDENT, (3, 3, 1)), active=active)


def case(name, make, bucket=8, eps=0.0, max_dist=INF, opts=None, engine=0, cond=()):
    return Case(name, make, bucket, eps, max_dist, dict(opts or {}), engine, tuple(cond))


def _cases():
    out = []

    def add(name, make, both=False, eps=(0.0, 3.16), cond=None, **kw):
        for e in eps:
            cd = (cond or {}).get(e, ()) if isinstance(cond, dict) else (cond or ())
            tag = f"{name}_eps{'0' if e == 0 else '316'}" if len(eps) > 1 else name
            out.append(case(tag, make, eps=e, cond=cd, **kw))
            if both:  # the same expectation on the node records
                out.append(case(tag + "_nodes", make, eps=e, cond=cd, opts=dict(nn_engine=1), engine=1, **kw))

    add("inside", make_inside, both=True, cond=("lds_only", "self_match"))
    add("outside_scratch", make_outside, both=True, cond={0.0: (("scratch_share", 0.5),), 3.16: (("scratch_count", 5),)})
    add("scale_small", functools.partial(make_outside, 2.0 ** -20), cond=("code_0",))
    add("scale_large", functools.partial(make_outside, 2.0 ** 20), cond=("code_255",))
    add("deep_line", make_deep_line, both=True,
        cond={0.0: (("depth", 47), ("unchecked_share", 0.25), ("nest", 20)), 3.16: (("depth", 47), ("unchecked_share", 0.25))})
    add("deep_ladder", make_deep_ladder, cond=(("unchecked_share", 0.25),))
    add("identical", make_identical, eps=(0.0,), cond=("ties",))
    add("lattice", make_lattice, eps=(0.0,), cond=("ties",))
    for r in (0.05, 0.5):
        add(f"radius_{str(r).replace('.', '')}", make_radius, max_dist=r, cond=("both_kinds",))
    for b in (1, 3, 15):
        add(f"bucket_{b}", make_buckets, bucket=b)
    add("bucket_16", make_buckets, bucket=16, engine=1)  # node records by rule
    add("saturate", make_saturate, eps=(0.0,), cond=("saturates",))
    add("transforms", make_transforms, eps=(3.16,))
    add("ragged_pairs", make_ragged_pairs, eps=(3.16,), cond=("rounds", "padding"))
    for shape in ((1, 1), (3, 1), (1, 65)):
        add(f"tiny_{shape[0]}x{shape[1]}", functools.partial(make_tiny, shape), eps=(3.16,), cond=("few_slots",))
    add("all_inactive", make_all_inactive, eps=(3.16,), cond=("idle_step",))
    return out


CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def inputs(make):
    """A case's inputs, built once and shared (read-only) by the cases on the same data."""
    inp = make()
    for a in inp.refs + inp.reads + (inp.T,) + (() if inp.active is None else (inp.active,)):
        a.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def _tree(make, r, bucket):
    import pyoracle as po

    return po.Tree(inputs(make).refs[r], bucket)


def oracle_tree(c, r):
    return _tree(c.make, r, c.bucket)


def queries(c, step, pair):
    inp = inputs(c.make)
    return transform(inp.T[step, pair], inp.reads[pair])


def is_active(c, step, pair):
    a = inputs(c.make).active
    return a is None or bool(a[step, pair])


@functools.lru_cache(maxsize=None)
def _expected(make, bucket, eps, max_dist):
    inp = inputs(make)
    S, P = inp.T.shape[:2]
    out = []
    for s in range(S):
        row = []
        for p in range(P):
            if inp.active is not None and not inp.active[s, p]:
                row.append(None)
                continue
            row.append(_tree(make, inp.pair_ref[p], bucket).nn1(transform(inp.T[s, p], inp.reads[p]), eps, max_dist))
        out.append(row)
    return out


def expected(c):
    """The oracle's per-query results of case c: [step][pair] -> Tree.nn1's dict (None: inactive).
    Computed once per (data, bucket, epsilon, max_dist) and shared; read-only."""
    return _expected(c.make, c.bucket, c.eps, c.max_dist)


def pooled(c, key):
    """One array of `key` over every query of every active pair and step of case c."""
    return np.concatenate([e[key] for row in expected(c) for e in row if e is not None])


def slots(c, step):
    """The NN launch's work space at a step: each active pair's readings padded to whole 64-slot
    chunks (k_active_list)."""
    inp = inputs(c.make)
    return sum((len(inp.reads[p]) + 63) // 64 * 64 for p in range(len(inp.reads)) if is_active(c, step, p))


# conditions on the reference alone; each returns (holds, the figure it rests on)
def _share(c, key, lo):
    v = pooled(c, key)
    return float((v >= lo).mean())


def _ties(c):
    inp = inputs(c.make)
    n = 0
    for p, e in enumerate(expected(c)[0]):
        d = brute_d2(inp.refs[inp.pair_ref[p]], queries(c, 0, p)[:64])
        n += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return n


def _self_match(c):
    e = expected(c)[0][1]  # the pair whose readings are the reference itself
    return bool(np.all(e["d2"] == 0) and np.array_equal(e["id"], np.arange(len(e["id"]))))


COND = {
    "lds_only": lambda c: (pooled(c, "nest").max() <= LDS_FRAMES, int(pooled(c, "nest").max())),
    "self_match": lambda c: (_self_match(c), None),
    "scratch_share": lambda c, lo: (_share(c, "nest", LDS_FRAMES + 1) >= lo, _share(c, "nest", LDS_FRAMES + 1)),
    "scratch_count": lambda c, lo: (int((pooled(c, "nest") > LDS_FRAMES).sum()) >= lo,
                                    int((pooled(c, "nest") > LDS_FRAMES).sum())),
    "code_0": lambda c: (0 < pooled(c, "max_bound").max() < PM_LO, float(pooled(c, "max_bound").max())),
    "code_255": lambda c: (pooled(c, "max_bound").max() > PM_HI, float(pooled(c, "max_bound").max())),
    "depth": lambda c, d: (oracle_tree(c, 0).info()[1] == d, oracle_tree(c, 0).info()[1]),
    "unchecked_share": lambda c, lo: (_share(c, "far_depth", POP_DEPTH) >= lo, _share(c, "far_depth", POP_DEPTH)),
    "nest": lambda c, lo: (pooled(c, "nest").max() >= lo, int(pooled(c, "nest").max())),
    "ties": lambda c: (_ties(c) > 0, _ties(c)),
    "both_kinds": lambda c: (0.05 <= float((pooled(c, "id") < 0).mean()) <= 0.99, float((pooled(c, "id") < 0).mean())),
    "saturates": lambda c: (int(pooled(c, "points")[1]) > SAT > int(pooled(c, "nodes")[1]) and
                            int(pooled(c, "points")[0]) < SAT,
                            (int(pooled(c, "points")[1]), int(pooled(c, "nodes")[1]))),
    "rounds": lambda c: (all(sum(is_active(c, s, p) for p in range(600)) > 256 for s in range(3)),
                         [sum(is_active(c, s, p) for p in range(600)) for s in range(3)]),
    "padding": lambda c: (any(len(r) == 1 for r in inputs(c.make).reads), None),
    "few_slots": lambda c: (slots(c, 0) < 512, slots(c, 0)),
    "idle_step": lambda c: (any(slots(c, s) == 0 for s in range(len(inputs(c.make).T))), None),
}


def check_cond(c, cond):
    name, args = (cond, ()) if isinstance(cond, str) else (cond[0], cond[1:])
    return COND[name](c, *args)
