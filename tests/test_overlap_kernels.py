"""The overlap kernels against exact voxel sets, key by key, on every production path.

Context.test_overlap (aicp_hip_test_overlap) runs the batch's own overlap (paths 0-2: grouping,
key boxes, overlap_maps or overlap_sparse) or the stream's window code (paths 3, 4: the plan and
the device steps sequence.cpp itself calls) on the clouds of overlap_reference.CASES and returns
what was written: every cloud's voxel map or sorted key words, the descriptors, the per-point key
counts, the counts, percentage and ratio. All of it is compared with the plain Python reference
(held to the C++ oracle ray by ray in test_overlap_reference.py). Every comparison is an equality.
"""
import numpy as np
import pytest

import overlap_reference as ov

pytestmark = pytest.mark.gpu
case_param = pytest.mark.parametrize("case", ov.CASES, ids=lambda c: c.name)
# the stream sizes a window's map slots on the host from the AABB of its finite points: a return of
# 5000 m or a finite coordinate of 1e30 puts the slots over the stream's 1 GiB budget, and the
# stream runs such a window on key lists (path 4); forced onto maps (path 3) the entry refuses it
NO_STREAM_MAPS = ("far_return", "invalid")


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


_RUNS = {}


def run(ctx, case, path, **kw):
    key = (case.name, path, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = ctx.test_overlap(case.refs, case.pair_ref, case.reads, case.ref_origins, case.read_origins,
                                      case.res, path=path, **kw)
    return _RUNS[key]


def diff(tag, got, want):
    """set equality, naming the first few missing and extra keys"""
    if got != want:
        miss, extra = sorted(want - got)[:6], sorted(got - want)[:6]
        print(tag, "missing", [ov.unpack(k) for k in miss], "extra", [ov.unpack(k) for k in extra])
    assert got == want, (tag, len(want - got), len(got - want))


def check_results(oracle, case, got):
    R, exp = ov.reference(case), ov.expected(case)
    tag = (case.name, got["path"])
    assert got["n_groups"] == R.G and got["pair_group"].tolist() == R.pair_group, tag
    assert got["cloud_keys"].tolist() == [len(S) for S in R.sets], tag
    assert not got["cloud_err"].any() and not got["pair_err"].any(), tag
    for c, (lo, hi) in enumerate(R.boxes):
        if got["path"] == 4:  # the key lists need no box: the stream leaves it at the origin's key
            lo, hi = ov.key_box([], R.clouds[c][1], case.res)
        assert got["cloud_bbox"][c].tolist() == lo + hi, (tag, c)
    for p, (n, pc, _) in enumerate(exp):
        assert tuple(got["pair_counts"][p].tolist()) == n, (tag, p)
        assert ov.same_f32(got["pair_percent"][p], pc), (tag, p, got["pair_percent"][p], pc)
        assert ov.same_f32(got["pair_ratio"][p], oracle.autotune_ratio(float(pc))), (tag, p, got["pair_ratio"][p])


def check_maps(case, got):
    R = ov.reference(case)
    tag = (case.name, got["path"])
    spans = []
    for c, S in enumerate(R.sets):
        mn, dim = ov.ovl_desc(*R.boxes[c])
        assert got["desc_min"][c].tolist() == mn and got["desc_dim"][c].tolist() == dim, (tag, c)
        off, nb = int(got["desc_off"][c]), int(got["desc_bytes"][c])
        assert nb == ov.ovl_bytes(dim) and off % 16 == 0 and off + nb <= got["arena_bytes"], (tag, c)
        spans.append((off, off + nb))
        diff((tag, "cloud", c), ov.decode_map(got["arena"][off:off + nb], mn, dim), S)
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), tag  # the maps do not overlap


def check_points(case, got):
    R = ov.reference(case)
    want = np.concatenate(R.counts)
    assert got["n_points"] == want.size and np.array_equal(got["key_counts"], want), (case.name, got["path"])
    return np.cumsum([0] + [len(c) for c in R.counts])


def check_words(tag, w, tags, sets):
    """a sorted list: the distinct words of tag t are t << 48 | key over sets[t]"""
    assert np.all(w[1:] >= w[:-1]), tag
    t = (w >> np.uint64(48)).astype(np.int64)
    k = w & np.uint64((1 << 48) - 1)
    for i, S in zip(tags, sets):
        diff((tag, "tag", i), set(k[t == i].tolist()), S)
    return t


def check_batch_keys(case, got):
    R = ov.reference(case)
    seg = check_points(case, got)
    total = int(seg.size and np.concatenate(R.counts).sum())
    assert got["n_words"] == total == got["words"].size, (case.name, got["n_words"], total)
    assert np.array_equal(got["key_offsets"], np.cumsum(np.concatenate(R.counts)) - np.concatenate(R.counts))
    t = check_words(case.name, got["words"], range(R.G + R.P), R.sets)
    assert t.size == 0 or t.max() < R.G + R.P


def check_stream_keys(case, got):
    R = ov.reference(case)
    seg = check_points(case, got)
    assert got["dirty"] == 0, case.name
    for g in range(R.G):
        members = [p for p in range(R.P) if R.pair_group[p] == g]
        for side, clouds in ((0, [R.G + p for p in members]), (1, [g])):
            n = len(clouds)
            off, cap = int(got["list_off"][2 * g + side]), int(got["list_cap"][2 * g + side])
            tag = (case.name, "window", g, "side", side)
            assert cap == int(sum(got["cloud_bound"][c] for c in clouds)), tag
            w = got["words"][off:off + cap]
            assert w.size == cap, tag
            t = check_words(tag, w, range(n), [R.sets[c] for c in clouds])
            total = int(sum(R.counts[c].sum() for c in clouds))
            assert total <= cap, tag  # the host's bound holds
            assert np.all(t[:total] < n) and np.all(w[total:] == np.uint64(n << 48)), tag  # then cap - total pad words
            cnt = np.concatenate([R.counts[c] for c in clouds])
            offs = np.concatenate([got["key_offsets"][seg[c]:seg[c + 1]] for c in clouds])
            assert np.array_equal(offs, np.cumsum(cnt) - cnt), tag
            for c in clouds:  # every cloud's own share holds its keys
                assert got["cloud_bound"][c] >= R.counts[c].sum(), (tag, c)


@case_param
def test_batch_maps(ctx, oracle, case):
    a, b = run(ctx, case, 1, filter=0, wide=0), run(ctx, case, 1, filter=1, wide=1)
    if case.name == "far_return":  # the size rule falls through to the sorted keys: not an error
        assert a["path"] == 2 and b["path"] == 2
        check_results(oracle, case, a)
        check_batch_keys(case, a)
        return
    for got, f in ((a, 0), (b, 1)):
        assert (got["path"], got["filter"], got["wide"]) == (1, f, f)
        check_results(oracle, case, got)
    check_maps(case, a)
    assert np.array_equal(a["arena"], b["arena"])  # the marks' cache changes no byte
    assert np.array_equal(a["pair_counts"], b["pair_counts"]) and np.array_equal(a["cloud_keys"], b["cloud_keys"])


@case_param
def test_batch_keys(ctx, oracle, case):
    got = run(ctx, case, 2)
    assert got["path"] == 2
    check_results(oracle, case, got)
    check_batch_keys(case, got)


@case_param
def test_stream_maps(L, ctx, oracle, case):
    if case.name in NO_STREAM_MAPS:
        rc = ctx.test_overlap(case.refs, case.pair_ref, case.reads, case.ref_origins, case.read_origins, case.res,
                              path=3, check=False)
        assert rc == L.AICP_ERR_UNSUPPORTED
        return
    a, b = run(ctx, case, 3), run(ctx, case, 3, filter=1, wide=1)
    assert (a["path"], a["filter"], a["wide"]) == (3, 0, 0) and (b["path"], b["filter"], b["wide"]) == (3, 1, 1)
    for got in (a, b):
        assert got["dirty"] == 0
        check_results(oracle, case, got)
    check_maps(case, a)
    assert np.array_equal(a["arena"], b["arena"])
    assert np.array_equal(a["pair_counts"], b["pair_counts"])
    for c in range(len(a["cloud_bound"])):  # the host's slot holds the map the device sized
        assert a["desc_bytes"][c] <= a["cloud_bound"][c]


@case_param
@pytest.mark.parametrize("rigid", (0, 1))
def test_stream_keys(ctx, oracle, case, rigid):
    got = run(ctx, case, 4, rigid=rigid, words_cap=16 << 20)
    assert got["path"] == 4
    check_results(oracle, case, got)
    check_stream_keys(case, got)


@case_param
def test_paths_agree(ctx, case):
    paths = [1, 2, 4] + ([] if case.name in NO_STREAM_MAPS else [3])
    runs = [run(ctx, case, 1, filter=0, wide=0), run(ctx, case, 2), run(ctx, case, 4, rigid=0, words_cap=16 << 20)]
    if 3 in paths:
        runs.append(run(ctx, case, 3))
    for got in runs[1:]:
        for k in ("pair_counts", "cloud_keys", "pair_group") + (("cloud_bbox",) if got["path"] != 4 else ()):
            assert np.array_equal(got[k], runs[0][k]), (case.name, k)
        for k in ("pair_percent", "pair_ratio"):
            assert np.array_equal(got[k].view(np.uint32), runs[0][k].view(np.uint32)), (case.name, k)


def test_batch_rules(ctx, oracle):
    """path 0: twelve clouds pick the marks' cache, one pair in one group the wide counts, a map
    above 2^34 voxels the sorted keys"""
    fan, one, far = (run(ctx, ov.BY_NAME[n], 0) for n in ("fan_filter", "lattice_0.2", "far_return"))
    assert (fan["path"], fan["filter"], fan["wide"]) == (1, 1, 0)
    assert (one["path"], one["filter"], one["wide"]) == (1, 0, 1)
    assert far["path"] == 2
    for name, got in (("fan_filter", fan), ("lattice_0.2", one), ("far_return", far)):
        check_results(oracle, ov.BY_NAME[name], got)
    check_maps(ov.BY_NAME["fan_filter"], fan)
    check_maps(ov.BY_NAME["lattice_0.2"], one)


def edge_window():
    """one window of small clouds: a 256-point reference, readings of 255, 257 and 2 points"""
    be = ov.BY_NAME["block_edges"]
    refs, reads = [be.refs[3]], [be.reads[2], be.reads[3], be.reads[4]]
    ro, do = [be.ref_origins[3]] * 3, [be.read_origins[2], be.read_origins[3], be.read_origins[4]]
    case = ov._case("edge_window", ov.RES, refs, reads, [0, 0, 0], ro, do, lambda R: None)
    return case, ov.reference(case)


def call(ctx, case, path, caps, **kw):
    return ctx.test_overlap(case.refs, case.pair_ref, case.reads, case.ref_origins, case.read_origins, case.res,
                            path=path, caps=caps, **kw)


def test_key_list_capacity_edges(ctx, oracle):
    case, R = edge_window()
    totals = [int(c.sum()) for c in R.counts]  # the reference, then the three readings
    for extra in (0, 1):  # cap == total: no pad word; total + 1: one per list
        got = call(ctx, case, 4, [t + extra for t in totals])
        check_results(oracle, case, got)
        check_stream_keys(case, got)
        assert got["list_cap"].tolist() == [sum(totals[1:]) + 3 * extra, totals[0] + extra]
        pads = [int((got["words"][int(o):int(o + c)] >> np.uint64(48) == n).sum())
                for o, c, n in zip(got["list_off"], got["list_cap"], (3, 1))]
        assert pads == [3 * extra, extra]
    sets = [len(S) for S in R.sets]
    # one word short. The readings share a list: the word that does not fit is the last reading's.
    got = call(ctx, case, 4, totals[:3] + [totals[3] - 1])
    assert got["cloud_err"].tolist() == [0, 0, 0, 1] and got["pair_err"].tolist() == [0, 0, 1]
    assert got["cloud_keys"][:3].tolist() == sets[:3] and got["dirty"] == 0
    for p in range(2):
        assert tuple(got["pair_counts"][p].tolist()) == ov.counts(R.sets[0], R.sets[1 + p])
    w = got["words"][int(got["list_off"][0]):][:int(got["list_cap"][0])]
    assert np.all(w[1:] >= w[:-1]) and np.all((w >> np.uint64(48)) < 3)  # full, no pad, nothing past cap (dirty)
    # the reference's own list one word short: its error reaches every pair, the readings' sets stay exact
    got = call(ctx, case, 4, [totals[0] - 1] + totals[1:])
    # (a reading's state is its pair's: k_ovl_finish folds the group's error into it)
    assert got["cloud_err"].tolist() == [1, 1, 1, 1] and got["pair_err"].tolist() == [1, 1, 1]
    assert got["cloud_keys"][1:].tolist() == sets[1:] and got["dirty"] == 0


def test_map_slot_capacity_edges(ctx, oracle):
    case, R = edge_window()
    nbytes = [ov.ovl_bytes(ov.ovl_desc(*b)[1]) for b in R.boxes]
    got = call(ctx, case, 3, nbytes)  # every slot exactly its map's bytes: fits
    check_results(oracle, case, got)
    check_maps(case, got)
    assert got["dirty"] == 0 and got["arena_bytes"] == sum(nbytes)
    caps = list(nbytes)
    caps[2] -= 128  # the second reading's slot one brick short
    got = call(ctx, case, 3, caps)
    assert got["cloud_err"].tolist() == [0, 0, 1, 0] and got["pair_err"].tolist() == [0, 1, 0] and got["dirty"] == 0
    assert got["desc_dim"][2].tolist() == [0, 0, 0] and got["desc_bytes"][2] == 0
    assert got["cloud_keys"][2] == 0 and got["pair_counts"][1].tolist() == [len(R.sets[0]), 0, 0]
    off = int(got["desc_off"][2])
    assert np.all(got["arena"][off:off + caps[2]] == 0xA5)  # the refused slot was never written
    for c in (0, 1, 3):  # the other maps are whole
        mn, dim = ov.ovl_desc(*R.boxes[c])
        o = int(got["desc_off"][c])
        diff(("slot", c), ov.decode_map(got["arena"][o:o + nbytes[c]], mn, dim), R.sets[c])
    for p in (0, 2):
        assert tuple(got["pair_counts"][p].tolist()) == ov.counts(R.sets[0], R.sets[1 + p])
