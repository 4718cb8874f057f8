"""The SurfaceNormal chain of a batch's references against exact references, point by point.

Context.test_normals (aicp_hip_test_normals) runs what a registration batch runs for its
references: the raw trees, launch_normals (the self-kNN k_knn_oct / k_knn_ids, then
k_normals_from_ids), the kNN once more with its touched counters, the matcher trees and
launch_normals_to_matcher, and downloads everything they wrote. Every case of
normals_reference.CASES runs under both kNN engines (and under the rule, normals_knn_engine 0,
where the case names the engine the rule must pick), and each run is held to the plain Python
references of normals_reference.py (auto_rule, 300 001 points: the C++ oracle's lists).
Equalities: every k-best list entry by entry (mapped to input ids, -1 where the list has no
entry), the second launch's lists, the touched points and inner nodes (the only witness that the
pruning is libnabo's), the two engines' outputs bit for bit, the matcher-order normal of every
input id bit for bit, both bucket orders being permutations, w = 0, no sentinel left and no guard
word changed. The normals themselves: normals_reference.check_normals, with the classes decided by
the exact covariance (rank <= 1: exactly e_y and counted per reference; regular: norm, Rayleigh
excess and sine within bounds derived from float32 rounding).

test_normals_reference.py (CPU) asserts on the reference alone that each case reaches what it is
there for. The nesting of far descents reached: deep_line 9 / 19 / 29, deep_ladder 15 / 22 / 29 and
deep_zigzag 13 / 32 / 32 at K = 10 / 20 / 30, every one past the per-lane engine's 6 LDS frames. The
octet engine's scratch frames (nesting > 24) are reached at K = 20 and 30: on a line and on the
ladder the nesting stops where the list is full (K - 1, K + 2), on the zig-zag ladder it goes on. It
is also the only case in which those frames' offsets and bounds show in the results (condition
frames_matter: on the line and the ladder a deep frame is popped straight into the next pop, and
only its node ids are read). For K = 10 no cloud within the 47-level limit was found whose nesting
passes 24 (largest found: 15, on the ladder).
"""
import ctypes as C

import numpy as np
import pytest

import normals_reference as nr
import tree_reference as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
MATCHER_BUCKET = 8  # (the registration's default bucket_size)


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture()
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_case(ctx, c, engine):
    """One run of case c under normals_knn_engine = engine, held to the reference. Returns what the
    device wrote, every per-point array in input order."""
    pts = nr.clouds(c.make)
    want, nis = nr.expected_knn(c), nr.inputs(c)
    with ctx.options(normals_knn_engine=engine):
        got = ctx.test_normals(pts, c.K, MATCHER_BUCKET)
    tag = f"{c.name} engine {engine}"
    assert got["engine"] == (engine or c.engine0), (tag, got["engine"])
    assert got["dirty"] == 0, (tag, got["dirty"])
    out = dict(ids=[], nrm=[], figs=[])
    for r, p in enumerate(pts):
        n = len(p)
        raw_id, matcher_id = got["raw_id"][r], got["matcher_id"][r]
        for perm in (raw_id, matcher_id):  # both bucket orders are permutations of the input
            assert np.array_equal(np.sort(perm), np.arange(n)), (tag, r)
        ids, ids2 = got["ids"][r], got["ids2"][r]
        assert np.all((ids >= -1) & (ids < n)), (tag, r, ids[(ids < -1) | (ids >= n)][:8])  # (no sentinel either)
        assert np.array_equal(ids2, ids), (tag, r, "second launch")
        by_input = np.empty_like(ids)
        by_input[raw_id] = np.where(ids >= 0, raw_id[np.maximum(ids, 0)], -1)
        bad = np.flatnonzero(np.any(by_input != want[r]["ids"], axis=1))
        assert bad.size == 0, (tag, r, bad.size, bad[:4].tolist(), by_input[bad[:4]].tolist(), want[r]["ids"][bad[:4]].tolist())
        nrm, bnrm = got["nrm"][r], got["bnrm"][r]
        for a in (nrm, bnrm):
            assert not np.any(bits(a) == nr.SENTINEL) and np.all(bits(a[:, 3]) == 0), (tag, r)
        nrm_in, bnrm_in = np.empty_like(nrm), np.empty_like(bnrm)
        nrm_in[raw_id] = nrm
        bnrm_in[matcher_id] = bnrm
        assert np.array_equal(bits(nrm_in), bits(bnrm_in)), (tag, r, "scatter")
        out["figs"].append(nr.check_normals(nis[r], nrm_in[:, :3], got["degenerate"][r], (tag, r)))
        out["ids"].append(by_input)
        out["nrm"].append(nrm_in)
    assert got["touched"] == (sum(w["points"] for w in want), sum(w["nodes"] for w in want)), (tag, got["touched"])
    figs = out["figs"]
    print(f"{tag}: " + ", ".join(f"{k} {max(f[k] for f in figs):.3f}" for k in ("norm", "excess", "sine")) +
          f", degenerate {int(got['degenerate'].sum())}, touched {got['touched']}")
    return out


@pytest.mark.parametrize("c", nr.CASES, ids=lambda c: c.name)
def test_case_equals_reference(ctx, c):
    runs = {e: run_case(ctx, c, e) for e in ((1, 2) if c.engine0 is None else (1, 2, 0))}
    for e in runs:  # the engines equal each other, bit for bit
        for r in range(len(runs[1]["ids"])):
            assert np.array_equal(runs[e]["ids"][r], runs[1]["ids"][r]), (c.name, e, r)
            assert np.array_equal(bits(runs[e]["nrm"][r]), bits(runs[1]["nrm"][r])), (c.name, e, r)


@pytest.mark.parametrize("engine", [1, 2])
def test_next_run_of_the_context_is_clean(ctx, engine):
    """The id scratch, the work counters, the per-reference degenerate counts and the trees carry
    nothing over: a batch of 300 references, six tiny ones, one deep tree and the 300 again."""
    for name in nr.CLEAN_CONTEXT:
        run_case(ctx, nr.by_name(name), engine)


def test_entry_refuses_bad_arguments(ctx, L):
    """Each refusal of aicp_hip_test_normals, one change away from a good call, and the good call
    again afterwards."""
    u32p, ip, up = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    n, K = 12, 10
    pts = tr.uniform(n, 5)
    base = dict(ctx=ctx.h, n_refs=1, counts=np.array([n], np.uint32), pts=pts, knn=K, bucket=8,
                ids=np.zeros(n * 30, np.int32), ids2=np.zeros(n * 30, np.int32), raw_id=np.zeros(n, np.int32),
                nrm=np.zeros(4 * n, f32), deg=np.zeros(1, np.int32), touched=np.zeros(2, np.uint64),
                bnrm=np.zeros(4 * n, f32), matcher_id=np.zeros(n, np.int32), engine=C.c_int32(), dirty=C.c_uint64())

    def call(**over):
        a = dict(base, **over)
        p = lambda k, t: None if a[k] is None else a[k].ctypes.data_as(t)
        f = lambda k: None if a[k] is None else L._fptr(a[k])
        return L.lib.aicp_hip_test_normals(
            a["ctx"], a["n_refs"], p("counts", u32p), f("pts"), a["knn"], a["bucket"], p("ids", ip), p("ids2", ip),
            p("raw_id", ip), f("nrm"), p("deg", ip), p("touched", up), f("bnrm"), p("matcher_id", ip),
            None if a["engine"] is None else C.byref(a["engine"]), None if a["dirty"] is None else C.byref(a["dirty"]))

    def good():
        assert call() == L.AICP_OK and base["engine"].value == 1 and base["dirty"].value == 0
        assert np.array_equal(np.sort(base["raw_id"]), np.arange(n)) and base["touched"][0] >= n

    good()
    bad = [dict(ctx=None)] + [{k: None} for k in ("counts", "pts", "ids", "ids2", "raw_id", "nrm", "deg", "touched", "bnrm",
                                                   "matcher_id", "engine", "dirty")]
    bad += [dict(n_refs=0), dict(n_refs=4097), dict(counts=np.array([0], np.uint32)),
            dict(counts=np.array([2 ** 28], np.uint32)), dict(bucket=0), dict(bucket=4097)]
    for b in bad:
        assert call(**b) == L.AICP_ERR_INVALID, list(b)
    for k in (0, 1, 9, 11, 25, 31, 64, -10):
        assert call(knn=k) == L.AICP_ERR_UNSUPPORTED, k
    assert call(knn=0, bucket=0) == L.AICP_ERR_INVALID  # (the invalid argument is reported first)
    good()
    # a raw tree of 48 levels: refused before anything searches it, and the context goes on
    over = np.ascontiguousarray(tr.clouds_of(tr.OVER_LIMIT.data)[0])
    m = len(over)
    big = dict(counts=np.array([m], np.uint32), pts=over, ids=np.zeros(m * K, np.int32), ids2=np.zeros(m * K, np.int32),
               raw_id=np.zeros(m, np.int32), nrm=np.zeros(4 * m, f32), bnrm=np.zeros(4 * m, f32),
               matcher_id=np.zeros(m, np.int32))
    assert call(**big) == L.AICP_ERR_UNSUPPORTED
    good()
    run_case(ctx, nr.by_name("tiny_k10"), 1)
