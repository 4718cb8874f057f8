"""The production NN search kernel against libnabo's recurseKnn, query by query.

Context.test_nn (aicp_hip_test_nn) builds the references' trees and treelets as a registration
batch does, then runs the active list and k_icp_nn with the production grid once per step and
downloads what every reading got. Every case of nn_reference.CASES is compared with the C++
oracle's per-query search (ao_tree_nn1) on the same float32 queries; test_nn_reference.py holds the
oracle to the plain Python traversal and asserts, on the reference alone, that each case reaches
the part of the kernel it is there for (scratch frames, frames below the pop check's depths, both
ends of the one-byte bound, touch-word saturation, padding slots, an active list built in several
rounds). All comparisons are equalities: the match mapped to its input id (-1: none), the distance
bit for bit, the touch word, the engine the case names, no guard word changed, and the sentinels
of every reading of an inactive pair.
"""
import ctypes as C

import numpy as np
import pytest

import nn_reference as nr

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture()
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def run_case(ctx, c):
    inp = nr.inputs(c.make)
    want = nr.expected(c)
    with ctx.options(**c.opts):
        got = ctx.test_nn(inp.refs, c.bucket, inp.pair_ref, inp.reads, inp.T, inp.active, c.eps, c.max_dist)
    assert got["engine"] == c.engine, (c.name, got["engine"])
    assert got["dirty"] == 0, (c.name, got["dirty"])
    for r, ids in enumerate(got["ids"]):  # the bucket order is a permutation of the input
        assert np.array_equal(np.sort(ids), np.arange(len(inp.refs[r]))), (c.name, r)
    S, P = inp.T.shape[:2]
    n_active = 0
    for s in range(S):
        for p in range(P):
            lo, hi = int(got["read_off"][p]), int(got["read_off"][p + 1])
            m, d2, tw = got["match"][s, lo:hi], got["d2"][s, lo:hi], got["touched"][s, lo:hi]
            tag = f"{c.name} step {s} pair {p}"
            e = want[s][p]
            if e is None:  # an inactive pair: nothing written
                assert np.all(m.view(np.uint32) == nr.SENTINEL) and np.all(d2.view(np.uint32) == nr.SENTINEL), tag
                assert np.all(tw == nr.TOUCH_SENTINEL), tag
                continue
            n_active += 1
            n_ref = len(inp.refs[inp.pair_ref[p]])
            assert np.all((m >= -1) & (m < n_ref)), (tag, m[(m < -1) | (m >= n_ref)][:8])
            ids = np.where(m >= 0, got["ids"][inp.pair_ref[p]][np.maximum(m, 0)], -1)
            for name, g, w in (("id", ids, e["id"]), ("d2", d2.view(np.uint32), e["d2"].view(np.uint32)),
                               ("touch", tw, nr.touch_word(e["nodes"], e["points"]))):
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, (tag, name, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist(),
                                       e["nest"][bad[:8]].tolist(), e["far_depth"][bad[:8]].tolist())
    return got, n_active


@pytest.mark.parametrize("c", nr.CASES, ids=lambda c: c.name)
def test_search_equals_oracle(ctx, c):
    run_case(ctx, c)


def test_next_search_of_the_context_is_clean(ctx):
    """The active list, the work counters and the result buffers carry nothing over: a many-pair
    case, a one-reading case and the many-pair case again in one context, then an idle step's."""
    for name in ("ragged_pairs", "tiny_1x1", "ragged_pairs", "all_inactive", "deep_line_eps0"):
        run_case(ctx, nr.by_name(name))


def test_entry_refuses_bad_arguments(ctx, L):
    """Each AICP_ERR_INVALID condition of aicp_hip_test_nn, and the good call they are one change
    away from."""
    u32p, ip, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    ref, rd = nr.inside(10, 1), nr.inside(4, 2)
    base = dict(ctx=ctx.h, n_refs=1, counts=np.array([10], np.uint32), ref=ref, bucket=8, n_pairs=2,
                pair_ref=np.array([0, 0], np.uint32), n_read=np.array([3, 1], np.uint32), rd=rd, n_steps=1,
                T=np.tile(nr.IDENT, (2, 1)), active=None, eps=0.0, max_dist=1.0,
                match=np.zeros(4, np.int32), d2=np.zeros(4, f32), touched=np.zeros(4, np.uint32),
                ids=np.zeros(10, np.int32), engine=C.c_int32(), dirty=C.c_uint64())

    def call(**over):
        a = dict(base, **over)
        u = lambda k: None if a[k] is None else a[k].ctypes.data_as(u32p)
        f = lambda k: None if a[k] is None else L._fptr(a[k])
        return L.lib.aicp_hip_test_nn(
            a["ctx"], a["n_refs"], u("counts"), f("ref"), a["bucket"], a["n_pairs"], u("pair_ref"), u("n_read"), f("rd"),
            a["n_steps"], f("T"), None if a["active"] is None else a["active"].ctypes.data_as(u8p), a["eps"],
            a["max_dist"], None if a["match"] is None else a["match"].ctypes.data_as(ip), f("d2"), u("touched"),
            None if a["ids"] is None else a["ids"].ctypes.data_as(ip),
            None if a["engine"] is None else C.byref(a["engine"]), None if a["dirty"] is None else C.byref(a["dirty"]))

    assert call() == L.AICP_OK and base["engine"].value == 0 and base["dirty"].value == 0
    assert call(max_dist=float("inf")) == L.AICP_OK
    bad = [dict(ctx=None)] + [{k: None} for k in ("counts", "ref", "pair_ref", "n_read", "rd", "T", "match", "d2",
                                                   "touched", "ids", "engine", "dirty")]
    bad += [dict(n_refs=0), dict(n_refs=4097), dict(n_pairs=0), dict(n_pairs=4097), dict(n_steps=0),
            dict(counts=np.array([0], np.uint32)), dict(n_read=np.array([3, 0], np.uint32)),
            dict(pair_ref=np.array([0, 1], np.uint32)), dict(bucket=0), dict(bucket=4097),
            dict(counts=np.array([2 ** 28], np.uint32)), dict(n_read=np.array([2 ** 28 - 1, 1], np.uint32)),
            dict(eps=-0.5), dict(eps=float("nan")), dict(max_dist=-1.0), dict(max_dist=float("nan")),
            dict(n_steps=2 ** 30)]  # (n_steps * total = 2^32)
    for b in bad:
        assert call(**b) == L.AICP_ERR_INVALID, list(b)
    assert call() == L.AICP_OK  # and the context still serves the good call
