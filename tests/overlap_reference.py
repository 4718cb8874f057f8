"""A plain reference of the octree overlap: key sets, counts, percentage, map layout, and the cases.

Pure Python / numpy, no device code and no oracle. octomap's known-voxel set of a cloud is every
key of computeRayKeys(origin, p) plus p's own key; the overlap is
min(|A & B| / |A|, |A & B| / |B|) * 100. Everything here is exact: sets of packed keys
k0 << 32 | k1 << 16 | k2, float32 bit patterns, byte maps.

test_overlap_reference.py (CPU) holds this module to the C++ oracle ray by ray and asserts that
every case reaches what it is there for; test_overlap_kernels.py (GPU) compares the device with it.
"""
import math
from types import SimpleNamespace

import numpy as np

f32 = np.float32
KMAX = 32768
DBL_MAX = 1.7976931348623157e308
RES = float(f32(0.2))  # YAMLConfigurator parses octomapResolution as<float>
BRICK = (8, 8, 2)
BRICK_BYTES = 128
EMPTY_LO, EMPTY_HI = 1 << 30, -(1 << 30)


# ------------------------------------------------------------------ keys and the walk --------
def key_checked(res, c):
    """coordToKeyChecked: floor((1 / res) * double(float32 c)) + 32768, None when outside
    [0, 65536) (NaN and +-inf included)."""
    v = (1.0 / res) * float(f32(c))
    if not math.isfinite(v):
        return None
    v = math.floor(v)
    if not (-KMAX <= v < KMAX):
        return None
    return int(v) + KMAX


def point_key(res, p):
    k = [key_checked(res, c) for c in p]
    return None if None in k else tuple(k)


def ray_keys(o, e, res, info=None):
    """computeRayKeys (float point3d, double DDA): the keys from the origin's up to, not including,
    the endpoint's. Nothing when either key is invalid or both are equal (the kernels' guards).
    info (a dict, optional) receives: zero_dir (a direction component is 0), moving (axes that
    move), mult (per step: how many moving axes share the smallest tMax), wrap (a key left
    [0, 65535] and wrapped, as octomap's 16-bit keys do)."""
    o = [f32(v) for v in o]
    e = [f32(v) for v in e]
    ko, ke = point_key(res, o), point_key(res, e)
    if info is not None:
        info.update(zero_dir=False, moving=0, mult=[], wrap=False)
    if ko is None or ke is None or ko == ke:
        return []
    out = [ko]
    with np.errstate(all="ignore"):
        d = [f32(e[i] - o[i]) for i in range(3)]
        nsq = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
        length = f32(math.sqrt(float(nsq)))
        d = [f32(v / length) for v in d]
    step, tmax, tdelta = [0] * 3, [0.0] * 3, [0.0] * 3
    cur = list(ko)
    for i in range(3):
        step[i] = 1 if d[i] > 0 else (-1 if d[i] < 0 else 0)
        if step[i]:
            vb = (float(cur[i] - KMAX) + 0.5) * res
            vb += float(f32(step[i] * res * 0.5))
            tmax[i] = (vb - float(o[i])) / float(d[i])
            tdelta[i] = res / float(abs(d[i]))
        else:
            tmax[i] = tdelta[i] = DBL_MAX
    if info is not None:
        info["zero_dir"] = 0 in step
        info["moving"] = sum(1 for s in step if s)
    ke = list(ke)
    flen = float(length)
    while True:
        if info is not None:
            m = min(tmax)
            info["mult"].append(sum(1 for i in range(3) if step[i] and tmax[i] == m))
        if tmax[0] < tmax[1]:
            dim = 0 if tmax[0] < tmax[2] else 2
        else:
            dim = 1 if tmax[1] < tmax[2] else 2
        c = cur[dim] + step[dim]
        if not 0 <= c <= 0xFFFF:
            if info is not None:
                info["wrap"] = True
            c &= 0xFFFF
        cur[dim] = c
        tmax[dim] += tdelta[dim]
        if cur == ke:
            break
        if min(tmax) > flen:
            break
        out.append(tuple(cur))
    return out


def pack(k):
    return (k[0] << 32) | (k[1] << 16) | k[2]


def unpack(k):
    k = int(k)
    return ((k >> 32) & 0xFFFF, (k >> 16) & 0xFFFF, k & 0xFFFF)


def cloud_set(points, origin, res, infos=None):
    """The known-voxel set of a cloud seen from origin (packed keys), and per point the number of
    keys its ray and endpoint contribute, duplicates included (what the key lists hold)."""
    o = np.asarray(origin, np.float64).astype(np.float32)
    S = set()
    counts = np.zeros(len(points), np.int64)
    for j, p in enumerate(points):
        info = {} if infos is not None else None
        ks = ray_keys(o, p, res, info)
        if infos is not None:
            infos.append(info)
        pk = [pack(k) for k in ks]
        if infos is not None:
            info["h"] = hash(tuple(pk))  # the ray's keys in order, for the ray-by-ray comparisons
        S.update(pk)
        ke = point_key(res, p)
        if ke is not None:
            S.add(pack(ke))
        counts[j] = len(ks) + (ke is not None)
    return S, counts


def key_box(points, origin, res):
    """Key box of the cloud's valid points and of its origin (when valid): (lo[3], hi[3]), the
    kernels' empty box when there is none."""
    lo, hi = [EMPTY_LO] * 3, [EMPTY_HI] * 3
    ks = [point_key(res, p) for p in points]
    ks.append(point_key(res, np.asarray(origin, np.float64).astype(np.float32)))
    for k in ks:
        if k is not None:
            lo = [min(a, b) for a, b in zip(lo, k)]
            hi = [max(a, b) for a, b in zip(hi, k)]
    return lo, hi


def ray_counts(origins, points, res):
    """cloud_set's per-point counts for many rays at once (origins, points: (n, 3) float32): the
    same walk on numpy arrays, one step of every unfinished ray per round, for the key_bound checks
    that walk every case under many motions. Rays over 1000 keys take the scalar walk."""
    O, P = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(points, np.float32)
    rf = 1.0 / res

    def keys(a):
        with np.errstate(all="ignore"):
            v = rf * a.astype(np.float64)
            fl = np.floor(v)
            ok = np.isfinite(v) & (fl >= -KMAX) & (fl < KMAX)
            return np.where(ok, fl, 0).astype(np.int64) + KMAX, ok.all(1)

    (ko, oko), (ke, oke) = keys(O), keys(P)
    cnt = oke.astype(np.int64)
    act = oko & oke & (ko != ke).any(1)
    longr = act & (np.abs(ke - ko).sum(1) > 1000)
    for j in np.flatnonzero(longr):
        cnt[j] += len(ray_keys(O[j], P[j], res))
    idx = np.flatnonzero(act & ~longr)
    if idx.size == 0:
        return cnt
    cnt[idx] += 1  # the origin's key
    o, e, ke, cur = O[idx], P[idx], ke[idx], ko[idx].copy()
    with np.errstate(all="ignore"):
        d = e - o
        nsq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        length = np.sqrt(nsq.astype(np.float64)).astype(np.float32)
        d = d / length[:, None]
        step = np.sign(d).astype(np.int64)
        vb = ((cur - KMAX) + 0.5) * res + (step * res * 0.5).astype(np.float32).astype(np.float64)
        d64 = d.astype(np.float64)
        tmax = np.where(step != 0, (vb - o.astype(np.float64)) / d64, DBL_MAX)
        tdelta = np.where(step != 0, res / np.abs(d64), DBL_MAX)
    flen = length.astype(np.float64)
    while idx.size:
        t0, t1, t2 = tmax[:, 0], tmax[:, 1], tmax[:, 2]
        dim = np.where(t0 < t1, np.where(t0 < t2, 0, 2), np.where(t1 < t2, 1, 2))
        r = np.arange(idx.size)
        cur[r, dim] = (cur[r, dim] + step[r, dim]) & 0xFFFF
        tmax[r, dim] += tdelta[r, dim]
        keep = ~((cur == ke).all(1) | (tmax.min(1) > flen))
        cnt[idx[keep]] += 1
        idx, ke, cur, step, tmax, tdelta, flen = (a[keep] for a in (idx, ke, cur, step, tmax, tdelta, flen))
    return cnt


# ------------------------------------------------------------------ results ------------------
def counts(A, B):
    return len(A), len(B), len(A & B)


def percent(nA, nB, nAB):
    """k_ovl_finish's float32 order: ov / |A|, ov / |B|, b < a ? b : a, * 100.0 in double, to float."""
    with np.errstate(all="ignore"):
        ov = f32(nAB)
        a, b = f32(ov / f32(nA)), f32(ov / f32(nB))
        mn = b if b < a else a
        return f32(float(mn) * 100.0)


def autotune_ratio(overlap_percent):
    """app.cpp:197-205: overlap / 100 clamped to [0.25, 0.70], through the chain file's text (%g)."""
    cur = f32(float(f32(overlap_percent)) / 100.0)
    if float(cur) < 0.25:
        cur = f32(0.25)
    elif float(cur) > 0.70:
        cur = f32(0.70)
    if cur != cur:
        return cur
    return f32(float("%g" % float(cur)))


def same_f32(a, b):
    """bit-equal float32 values, any NaN equal to any NaN"""
    a, b = f32(a), f32(b)
    return bool((a != a and b != b) or a.view(np.uint32) == b.view(np.uint32))


# ------------------------------------------------------------------ map layout ---------------
def ovl_axis(lo, hi, b):
    """the padded, brick-aligned box of keys [lo, hi] on an axis of brick extent b: (min, dim)"""
    if lo > hi:
        lo = hi = 0
    l, h = lo - 2, hi + 3
    mn = (l // b) * b
    return mn, ((h - mn) + b - 1) // b * b


def ovl_desc(lo, hi):
    ax = [ovl_axis(lo[k], hi[k], BRICK[k]) for k in range(3)]
    return [a[0] for a in ax], [a[1] for a in ax]


def ovl_bytes(dim):
    return dim[0] * dim[1] * dim[2]


def ovl_index(a, b, c, dim1, dim2):
    brick = ((a >> 3) * (dim1 >> 3) + (b >> 3)) * (dim2 >> 1) + (c >> 1)
    return brick * BRICK_BYTES + (((a & 7) << 4) | ((b & 7) << 1) | (c & 1))


def encode_map(S, mn, dim):
    m = np.zeros(ovl_bytes(dim), np.uint8)
    for k in S:
        k = unpack(k)
        a, b, c = k[0] - mn[0], k[1] - mn[1], k[2] - mn[2]
        assert 0 <= a < dim[0] and 0 <= b < dim[1] and 0 <= c < dim[2], (k, mn, dim)
        m[ovl_index(a, b, c, dim[1], dim[2])] = 1
    return m


def decode_map(m, mn, dim):
    """the set of packed keys whose byte is 1; every byte must be 0 or 1 (the popcounts rely on it)"""
    m = np.asarray(m, np.uint8)
    assert m.size == ovl_bytes(dim), (m.size, dim)
    assert int(m.max(initial=0)) <= 1, "a map byte is neither 0 nor 1"
    idx = np.flatnonzero(m).astype(np.int64)
    brick, w = idx // BRICK_BYTES, idx % BRICK_BYTES
    b1, b2 = dim[1] >> 3, dim[2] >> 1
    a = (brick // (b1 * b2)) * 8 + (w >> 4) + mn[0]
    b = ((brick // b2) % b1) * 8 + ((w >> 1) & 7) + mn[1]
    c = (brick % b2) * 2 + (w & 1) + mn[2]
    assert a.size == 0 or (min(a.min(), b.min(), c.min()) >= 0 and max(a.max(), b.max(), c.max()) <= 0xFFFF)
    return set(((a << 32) | (b << 16) | c).tolist())


def key_end_bit(n_clouds):
    """the stream's key lists are sorted on bits [0, end): 48 key bits, the cloud tag, the pad tag"""
    b = 1
    while (1 << b) <= n_clouds:
        b += 1
    return 48 + b


def mark_slot(v):
    """k_ovl_mark's 12-bit cache slot of a voxel index"""
    return ((v * 2654435761) & 0xFFFFFFFF) >> 20


# ------------------------------------------------------------------ cases --------------------
def scan(n, seed, origin, half=3.0):
    """an ordinary cloud: returns within `half` metres of the origin, flatter in z"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-half, half, (n, 3)) * np.array([1.0, 1.0, 0.3])
    return (p + np.asarray(origin, np.float64)).astype(np.float32)


def _case(name, res, refs, reads, pair_ref, ref_origins, read_origins, cond, **aux):
    return SimpleNamespace(name=name, res=float(res), refs=[np.ascontiguousarray(r, np.float32) for r in refs],
                           reads=[np.ascontiguousarray(r, np.float32) for r in reads], pair_ref=list(pair_ref),
                           ref_origins=np.asarray(ref_origins, np.float64).reshape(-1, 3),
                           read_origins=np.asarray(read_origins, np.float64).reshape(-1, 3), cond=cond,
                           aux=SimpleNamespace(**aux))


_REF = {}


def reference(case):
    """The case's sets, built once: groups (reference, origin) in order of first appearance, then
    readings. Returns a namespace: groups [(ref, origin)], pair_group, clouds [(points, origin)],
    sets, counts (per point), infos (per ray), boxes (lo, hi), G, P."""
    if case.name in _REF:
        return _REF[case.name]
    groups, pair_group = [], []
    for p, r in enumerate(case.pair_ref):
        g = (r, tuple(case.ref_origins[p].tolist()))
        if g not in groups:
            groups.append(g)
        pair_group.append(groups.index(g))
    clouds = [(case.refs[r], np.array(o)) for r, o in groups]
    clouds += [(case.reads[p], case.read_origins[p]) for p in range(len(case.reads))]
    sets, cnts, infos, boxes = [], [], [], []
    for pts, org in clouds:
        inf = []
        S, c = cloud_set(pts, org, case.res, inf)
        sets.append(S)
        cnts.append(c)
        infos.append(inf)
        boxes.append(key_box(pts, org, case.res))
    R = SimpleNamespace(groups=groups, pair_group=pair_group, clouds=clouds, sets=sets, counts=cnts, infos=infos,
                        boxes=boxes, G=len(groups), P=len(case.reads))
    _REF[case.name] = R
    return R


def _all_infos(R):
    return [i for inf in R.infos for i in inf]


def _lattice(res, tag):
    h = res / 2
    deltas = []
    for n in range(1, 13):
        for ax in range(3):
            for s in (1, -1):
                d = [0, 0, 0]
                d[ax] = s * n
                deltas.append(d)  # axis-aligned: two zero direction components
        for ax in range(3):
            for s in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                d = [0, 0, 0]
                d[(ax + 1) % 3], d[(ax + 2) % 3] = s[0] * n, s[1] * n
                deltas.append(d)  # plane diagonals: endpoints on edges and corners, tMax ties
        for s in range(8):
            deltas.append([n * (1 if s & 1 else -1), n * (1 if s & 2 else -1), n * (1 if s & 4 else -1)])
    rng = np.random.default_rng(11)
    deltas += rng.integers(-24, 25, (300, 3)).tolist()
    deltas = np.array(deltas, np.int64)
    o_ref = np.array([3, 3, 3])    # a voxel centre, the same coordinate on every axis (exact ties)
    o_read = np.array([0, 4, -6])  # on three voxel faces
    lat = lambda idx: (idx.astype(np.float64) * h).astype(np.float32)

    def cond(R):
        inf = _all_infos(R)
        assert sum(1 for i in inf if i["zero_dir"]) >= 50
        assert sum(1 for i in inf if any(m >= 2 for m in i["mult"])) >= 50

    return _case("lattice_" + tag, res, [lat(o_ref + deltas)], [lat(o_read + deltas)], [0],
                 [lat(o_ref).astype(np.float64)], [lat(o_read).astype(np.float64)], cond)


def _diagonals():
    res = 0.25  # a power of two: centres, endpoints and directions are exact
    dirs = [(a, b, 0) for a in (1, -1) for b in (1, -1)]
    dirs += [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    d = np.array([[n * v for v in dr] for dr in dirs for n in range(1, 41)], np.float64) * res
    o_ref, o_read = np.array([0.625, 0.625, 0.625]), np.array([-1.125, 0.375, 2.125])

    def cond(R):
        for i in _all_infos(R):
            m = i["moving"]
            assert m in (2, 3) and i["mult"]
            # the walk takes the axes of a tie one after the other: each round starts with all tied
            assert all(v == m for v in i["mult"][::m]), i

    return _case("diagonals", res, [o_ref + d], [o_read + d], [0], [o_ref], [o_read], cond)


def _same_voxel():
    rng = np.random.default_rng(12)
    refs, reads, orgs = [], [], []
    for o in ((0.31, 0.52, -0.27), (-0.45, 0.11, 0.07)):
        o = np.array(o)
        base = np.floor(o / RES) * RES
        inside = base + rng.uniform(0.02, RES - 0.02, (30, 3))
        pts = np.concatenate([inside, np.repeat(o[None], 5, 0), scan(40, 13, o)]).astype(np.float32)
        (refs if not refs else reads).append(pts)
        orgs.append(o.astype(np.float32).astype(np.float64))

    def cond(R):
        for c in R.counts:
            assert int((c == 1).sum()) >= 20

    return _case("same_voxel", RES, refs, reads, [0], [orgs[0]], [orgs[1]], cond)


def _invalid():
    lim = KMAX * RES
    nan, inf = float("nan"), float("inf")
    bad = []
    for ax in range(3):
        for v in (nan, inf, -inf, lim * 1.5, -lim * 1.5, float(f32(lim)) * 2, 1e30, -1e30):
            p = [0.5, -0.4, 0.2]
            p[ax] = v
            bad.append(p)
    bad = np.array(bad, np.float32)
    o0, o1 = np.array([0.1, 0.2, 0.3]), np.array([0.6, -0.3, 0.25])
    ref0 = np.concatenate([scan(150, 21, o0)[:75], bad, scan(150, 21, o0)[75:]])
    read0 = np.concatenate([bad[::2], scan(200, 22, o1), bad[1::2]])
    # the exact boundary values, from origins next to them (small key boxes)
    lo_v, hi_v = f32(-lim), np.nextafter(f32(lim), f32(0))
    o_lo, o_hi = np.full(3, -lim + 2.0), np.full(3, lim - 2.0)
    ref1, read1 = scan(60, 23, o_lo, 1.5), scan(60, 24, o_hi, 1.5)
    for ax in range(3):
        ref1[ax, ax], read1[ax, ax] = lo_v, hi_v
    empty = bad.copy()

    def cond(R):
        assert R.G == 4 and R.P == 4
        nb = len(bad)
        assert not R.counts[0][75:75 + nb].any() and not R.counts[4][:(nb + 1) // 2].any()  # the bad points of pair 0
        assert R.counts[0][:75].all() and R.counts[4][(nb + 1) // 2:(nb + 1) // 2 + 200].all()
        for c in (3, 6):  # the cloud without a valid point, as a reference and as a reading
            assert len(R.sets[c]) == 0 and not R.counts[c].any()

    return _case("invalid", RES, [ref0, ref1, ref0[:75], empty], [read0, read1, empty, read0[12:212]], [0, 1, 2, 3],
                 [o0, o_lo, o0, o0], [o1, o_hi, o1, o1], cond)


def _key_edge():
    lim = KMAX * RES
    clouds, orgs = [], []
    for sgn, seed in ((-1, 31), (-1, 32), (1, 33), (1, 34)):
        o = sgn * (lim - np.array([3.0, 4.0, 2.5]) - (seed % 2))
        p = scan(300, seed, o, 5.0).astype(np.float64)
        p = np.clip(p, -lim + 0.01, lim - 0.01)
        edge = np.tile(o, (6, 1))
        for ax in range(3):  # returns in the outermost voxel and in the one next to it, per axis
            edge[2 * ax, ax] = sgn * (lim - 0.5 * RES)
            edge[2 * ax + 1, ax] = sgn * (lim - 1.5 * RES)
        clouds.append(np.concatenate([p, edge]).astype(np.float32))
        orgs.append(o)

    def cond(R):
        assert not any(i["wrap"] for i in _all_infos(R))
        seen = set()
        for S in R.sets:
            for k in S:
                seen.update(unpack(k))
        assert {0, 1, 65534, 65535} <= seen

    return _case("key_edge", RES, [clouds[0], clouds[2]], [clouds[1], clouds[3]], [0, 1], [orgs[0], orgs[2]],
                 [orgs[1], orgs[3]], cond)


def _brick_offsets():
    o_a, o_b, o_c = np.array([0.1, 0.1, 0.1]), np.array([1.5, -2.0, 0.4]), np.array([-0.7, 0.9, -0.1])
    ref0, ref1 = scan(1024, 41, o_a, 4.0), scan(500, 42, o_c, 3.0)
    centres = [(-4.4, -4.4, -1.4), (4.4, 4.4, 1.4), (-4.4, 4.4, 0.3), (0.5, -0.7, 0.1), (30.0, 30.0, 5.0)]
    reads, ro = [], []
    for i, c in enumerate(centres):
        c = np.array(c)
        reads.append(scan(300, 43 + i, c, 1.5))
        ro.append(c + np.array([0.05, -0.03, 0.02]))
    # reading 3 also sees the reference's lowest return on each axis: its box starts where the reference's does
    reads[3] = np.concatenate([reads[3], ref0[np.argmin(ref0, axis=0)]])
    reads += [scan(300, 50, o_b, 2.0), scan(300, 51, o_c, 2.0)]
    ro += [o_b + 0.3, o_c - 0.2]

    def cond(R):
        assert R.G == 3 and R.P == 7 and R.pair_group == [0, 0, 0, 0, 0, 1, 2]
        a_mn, a_dim = ovl_desc(*R.boxes[0])
        signs, below, above = [set(), set(), set()], [False] * 3, [False] * 3
        for p in range(5):
            b_mn, b_dim = ovl_desc(*R.boxes[R.G + p])
            for k in range(3):
                o = (b_mn[k] - a_mn[k]) // BRICK[k]
                assert (b_mn[k] - a_mn[k]) % BRICK[k] == 0
                signs[k].add((o > 0) - (o < 0))
                below[k] |= b_mn[k] < a_mn[k] and R.boxes[R.G + p][1][k] >= a_mn[k]
                above[k] |= b_mn[k] + b_dim[k] > a_mn[k] + a_dim[k] and b_mn[k] < a_mn[k] + a_dim[k]
        assert all(s == {-1, 0, 1} for s in signs), signs
        assert all(below) and all(above)
        assert len(R.sets[0] & R.sets[R.G + 4]) == 0 and len(R.sets[0] & R.sets[R.G + 3]) > 0

    return _case("brick_offsets", RES, [ref0, ref1], reads, [0, 0, 0, 0, 0, 0, 1], [o_a] * 5 + [o_b, o_c], ro, cond)


def _fan(seed, origin):
    """a sensor-like fan of 1792 short rays, 256 consecutive ones inside a 51-degree wedge on 4
    rings, then one workgroup's worth of long rays over the whole sphere (thousands of distinct
    voxels for the 4096 slots of the marks' cache)"""
    rng = np.random.default_rng(seed)
    j = np.arange(1792)
    az = (j // 4) * (2 * np.pi / 448) + rng.uniform(0, 1e-3, j.size)
    el = ((j % 4) - 1.5) * 0.08
    r = rng.uniform(2.0, 3.0, j.size)
    fan = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)
    v = rng.normal(size=(256, 3))
    far = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(8.0, 10.0, (256, 1))
    return (np.concatenate([fan, far]) + origin).astype(np.float32)


def _fan_filter():
    orgs = [np.array([0.3 * i, -0.2 * i, 0.05 * i]) for i in range(12)]
    clouds = [_fan(60 + i, o) for i, o in enumerate(orgs)]

    def cond(R):
        assert R.G + R.P == 12  # above the batch's threshold of 8 clouds for the cache
        best = 0
        for (pts, org), S, cnt, box in zip(R.clouds, R.sets, R.counts, R.boxes):
            fan_set, fan_cnt = cloud_set(pts[:1792], org, RES)
            assert fan_cnt.sum() / len(fan_set) >= 8  # the fan's mean duplicates per voxel
            mn, dim = ovl_desc(*box)
            o32 = np.asarray(org, np.float64).astype(np.float32)
            vox = set()
            for p in pts[-256:]:  # the last workgroup's rays
                ks = ray_keys(o32, p, RES) + [point_key(RES, p)]
                vox.update(ovl_index(k[0] - mn[0], k[1] - mn[1], k[2] - mn[2], dim[1], dim[2]) for k in ks)
            best = max(best, len(vox) - len({mark_slot(v) for v in vox}))
        assert best >= 1000, best  # distinct voxels of one workgroup beyond the first in their slot

    return _case("fan_filter", RES, clouds[:6], clouds[6:], range(6), orgs[:6], orgs[6:], cond)


def _block_edges():
    o = [np.array([0.2 * i, 0.1 * i, 0.0]) for i in range(10)]
    n_ref, n_read = [2048, 1, 2, 256, 513], [1, 2048, 255, 257, 2]
    refs = [scan(n, 70 + i, o[i]) for i, n in enumerate(n_ref)]
    reads = [scan(n, 80 + i, o[5 + i]) for i, n in enumerate(n_read)]
    return _case("block_edges", RES, refs, reads, range(5), o[:5], o[5:], lambda R: None)


def _far_return():
    o0, o1 = np.array([0.0, 0.0, 0.5]), np.array([0.4, 0.3, 0.5])
    read = np.concatenate([scan(1500, 91, o1), np.array([[5000.0, 5000.0, 5000.0]], np.float32)])

    def cond(R):
        assert int(R.counts[1][-1]) > 60000
        _, dim = ovl_desc(*R.boxes[1])
        assert ovl_bytes(dim) > 1 << 34  # the dense size rule rejects the reading's map

    return _case("far_return", RES, [scan(1500, 90, o0)], [read], [0], [o0], [o1], cond)


def _many_clouds(n):
    o = np.array([0.1, -0.1, 0.2])
    reads = [scan(300, 100 + 10 * n + i, o + 0.15 * (i + 1)) for i in range(n)]
    ro = [o + 0.15 * (i + 1) for i in range(n)]
    return _case(f"many_clouds_{n}", RES, [scan(300, 99, o)], reads, [0] * n, [o] * n, ro, lambda R: None)


MANY = (1, 2, 3, 4, 7, 8)
CASES = [_lattice(RES, "0.2"), _lattice(0.05, "0.05"), _lattice(1.0, "1.0"), _diagonals(), _same_voxel(), _invalid(),
         _key_edge(), _brick_offsets(), _fan_filter(), _block_edges(), _far_return()] + [_many_clouds(n) for n in MANY]
BY_NAME = {c.name: c for c in CASES}
ORDINARY = ("brick_offsets", "block_edges", "many_clouds_8", "fan_filter")  # sensor-like clouds, no hard rays


def expected(case):
    """Per pair of the case: (|A|, |B|, |A & B|), the percentage and the ratio model."""
    R = reference(case)
    out = []
    for p in range(R.P):
        n = counts(R.sets[R.pair_group[p]], R.sets[R.G + p])
        pc = percent(*n)
        out.append((n, pc, autotune_ratio(pc)))
    return out
