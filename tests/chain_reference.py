"""Plain-numpy restatement of the sampled chains: the draw, libpointmatcher's MinDist,
RandomSampling and MaxDensity data-point filters, and a whole point-to-plane run on filtered clouds.
The reference of test_chain_cpu.py, test_chain_filters.py and test_chain_registration.py.

The draw. uniform(seed, slot, i) = k 2^-24, k the top 24 bits of two splitmix64 finaliser rounds
over seed, slot and i (chain_draw.hpp), in numpy uint64 arithmetic. slot = 4 side + the filter's
position in its list; i = the point's index in the cloud as that filter receives it.

The filters, each keeping its input's order:
  MinDist         dim -1: sqrt((x x + y y) + z z) > |minDist| in float32, one rounding per operation;
                  dim 0..2: |coord| > minDist
  RandomSampling  uniform < prob; every point draws
  MaxDensity      density <= maxDensity: kept, no draw. Otherwise accept = maxDensity / density,
                  times (1 - nbSaturated // nbPointsIn) for the points whose density equals the
                  cloud's maximum; kept when uniform < accept
The densities are an input: the device's own (checked on their own against the oracle's), or the
oracle's where the reference stands alone.

simulate() makes "device outputs" from the reference itself, optionally with one of MUTATIONS built
in; compare() checks device outputs against the reference; CASES is the table the GPU tests run.
"""
import functools
import math

import numpy as np

import p2p_reference as pr
import step_reference as sr
from step_reference import MarginError, Mismatch, f32, f64

SN, MIN_DIST, RANDOM, MAX_DENSITY = 1, 2, 3, 4   # AICP_FILTER_*
REFERENCE, READING = 0, 1
MUTATIONS = ("ge", "draw_out_index", "draw_all", "float_saturation", "order")
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


# ------------------------------------------------------------------ the draw ---------------
def mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def uniform(seed, slot, i):
    """float32 array of the draws of indices i (any integer array below 2^32)."""
    i = np.asarray(i, np.uint64)
    with np.errstate(over="ignore"):
        a = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + _GOLD * np.uint64(slot + 1))
        b = mix64(a + _GOLD * (i + np.uint64(1)))
    return ((b >> np.uint64(40)).astype(np.uint32).astype(f32) * f32(2.0 ** -24)).astype(f32)


# ------------------------------------------------------------------ the filters ------------
def min_dist_keep(pts, dim=-1, min_dist=1.0, mut=None):
    p = np.asarray(pts, f32)
    with np.errstate(all="ignore"):
        if dim < 0:
            v = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
            lim = f32(abs(f32(min_dist)))
        else:
            v = np.abs(p[:, dim])
            lim = f32(min_dist)
        assert v.dtype == f32
        return v >= lim if mut == "ge" else v > lim


def _draws(n, seed, slot, decide, mut):
    """keep[i] = decide(i, r_i). The draw's index is i; under draw_out_index, the point's position in
    the output so far (what a sequential stream that advances per kept point would do)."""
    if mut != "draw_out_index":
        r = uniform(seed, slot, np.arange(n))
        return np.array([decide(i, r[i]) for i in range(n)], bool)
    keep = np.zeros(n, bool)
    k = 0
    for i in range(n):
        keep[i] = decide(i, uniform(seed, slot, np.array([k]))[0])
        k += int(keep[i])
    return keep


def random_keep(n, prob, seed, slot, mut=None):
    p = f32(prob)
    return _draws(n, seed, slot, lambda i, r: bool(r < p), mut)


def max_density_keep(dens, max_density, seed, slot, mut=None):
    d = np.asarray(dens, f32)
    n = len(d)
    md = f32(max_density)
    with np.errstate(all="ignore"):
        last = f32(-np.inf)
        for v in d:       # the maximum by >, as the device takes it (NaN never wins)
            if v > last:
                last = v
        n_sat = int(np.sum(d == last))
        if mut == "float_saturation":
            factor = f32(1.0 - n_sat / n)
        else:
            factor = f32(1 - n_sat // n)

        def decide(i, r):
            if not (d[i] > md) and mut != "draw_all":
                return True
            accept = f32(md / d[i])
            if d[i] == last:
                accept = f32(accept * factor)
            return bool(r < accept)

        return _draws(n, seed, slot, decide, mut)


def run_filters(pts, filters, side, seed, densities=None, mut=None):
    """One side's list on one cloud. filters: dicts with `kind` and that kind's parameters;
    densities: of the cloud at the SurfaceNormal with keep_densities (None: the oracle's).
    Returns dict(index (kept input indices, in output order), counts (after each filter), sn_n (the
    cloud's size at the SurfaceNormal, None without one), sn_index (its input indices))."""
    pts = np.ascontiguousarray(pts, f32)[:, :3]
    idx = np.arange(len(pts))
    dens = None
    out = dict(counts=[], sn_n=None, sn_index=None)
    for pos, f in enumerate(filters):
        slot = 4 * side + pos
        kind = f["kind"]
        if kind == SN:
            out["sn_n"], out["sn_index"] = len(idx), idx.copy()
            if f.get("keep_densities"):
                if densities is None:
                    import pyoracle as po

                    dens = po.surface_normals(pts[idx], f["knn"])[1] if len(idx) else np.zeros(0, f32)
                else:
                    dens = np.asarray(densities, f32)
                    assert len(dens) == len(idx), (len(dens), len(idx))
            keep = np.ones(len(idx), bool)
        elif kind == MIN_DIST:
            keep = min_dist_keep(pts[idx], f.get("dim", -1), f.get("min_dist", 1.0), mut)
        elif kind == RANDOM:
            keep = random_keep(len(idx), f.get("prob", 0.75), seed, slot, mut)
        elif kind == MAX_DENSITY:
            keep = max_density_keep(dens, f.get("max_density", 10.0), seed, slot, mut)
        else:
            raise ValueError(kind)
        idx = idx[keep]
        if dens is not None:
            dens = dens[keep]
        out["counts"].append(len(idx))
    if mut == "order" and len(idx) > 1:
        idx = np.r_[idx[1], idx[0], idx[2:]]
    out["index"] = idx.astype(np.int32)
    return out


def make_chain(L, ref_filters=(), read_filters=(), seed=0, max_dist_d2=None):
    """The aicp_chain (aicp_mapping_amd._lib.Chain) of two filter lists."""
    ch = L.Chain()
    for side, fl in ((REFERENCE, ref_filters), (READING, read_filters)):
        for f in fl:
            ch.add(side, f["kind"], **{k: v for k, v in f.items() if k != "kind"})
    ch.seed = seed
    if max_dist_d2 is not None:
        ch.outlier = L.AICP_OUTLIER_MAX_DIST
        ch.outlier_limit_d2 = max_dist_d2
    return ch


# ------------------------------------------------------------------ the cases ---------------
COMPACT_N = (1, 255, 256, 257, 1023, 1024, 1025, 4097)
RADIUS = 2.5   # (1.5, 2, 0) has norm exactly 2.5: 2.25 + 4 = 6.25, every step exact in float32


def _pattern_cloud(n, keep):
    """n points whose MinDist(2.5) keep pattern is `keep`: kept ones at norm 5 (3, 4, 0 scaled by
    powers of two and signs), dropped ones exactly on the radius (1.5, 2, 0) or inside it."""
    rng = np.random.default_rng(n)
    pts = np.zeros((n, 3), f32)
    for i in range(n):
        sgn = rng.choice([-1.0, 1.0], 3)
        perm = rng.permutation(3)
        if keep[i]:
            v = np.array([3.0, 4.0, 0.0]) * 2.0 ** int(rng.integers(0, 3))
        elif i % 2:
            v = np.array([1.5, 2.0, 0.0])            # on the radius: > drops it, >= keeps it
        else:
            v = np.array([0.6, 0.8, 0.0]) * 2.0 ** int(rng.integers(-2, 1))   # norm 0.25 .. 1, inside
        pts[i] = (v * sgn)[perm]
    return pts


def _compaction_cases():
    out = {}
    for n in COMPACT_N:
        pats = dict(none=np.zeros(n, bool), all=np.ones(n, bool), alt=np.arange(n) % 2 == 0)
        if n == 1025:
            first = np.zeros(n, bool)
            first[0] = True
            last = np.zeros(n, bool)
            last[-1] = True
            pats.update(first=first, last=last)
        for name, keep in pats.items():
            out[f"compact_{n}_{name}"] = dict(pts=_pattern_cloud(n, keep), side=READING, seed=0,
                                              filters=[dict(kind=MIN_DIST, dim=-1, min_dist=RADIUS)], want=keep)
    return out


def _axis_cases():
    """|coord| == minDist exactly, just above and just below, for dim 0..2 (n = 300)."""
    out = {}
    for dim in range(3):
        rng = np.random.default_rng(70 + dim)
        pts = rng.uniform(-4, 4, (300, 3)).astype(f32)
        c = pts[:, dim]
        c[0::3] = f32(1.25) * rng.choice([-1, 1], len(c[0::3]))
        c[1::3] = np.nextafter(f32(1.25), f32(2)) * rng.choice([-1, 1], len(c[1::3]))
        c[2::3] = np.nextafter(f32(1.25), f32(0)) * rng.choice([-1, 1], len(c[2::3]))
        want = np.zeros(300, bool)
        want[1::3] = True
        out[f"axis_{dim}"] = dict(pts=pts, side=REFERENCE, seed=0, filters=[dict(kind=MIN_DIST, dim=dim, min_dist=1.25)],
                                  want=want)
    return out


def _random_cases():
    out = {}
    rng = np.random.default_rng(81)
    pts = rng.uniform(-6, 6, (4097, 3)).astype(f32)
    for prob in (0.0, 1.0, 0.05, 0.5):
        for seed in (0, 12345):
            out[f"random_{prob}_{seed}"] = dict(pts=pts, side=READING, seed=seed, filters=[dict(kind=RANDOM, prob=prob)])
    # the draw's index is the position after MinDist
    out["mindist_random"] = dict(pts=pts, side=REFERENCE, seed=3,
                                 filters=[dict(kind=MIN_DIST, min_dist=4.0), dict(kind=RANDOM, prob=0.5)])
    return out


CUBE8 = np.array([[a, b, c] for a in (-0.5, 0.5) for b in (-0.5, 0.5) for c in (-0.5, 0.5)], f32)
CUBE8_DENSITY = 2.940421   # of every point (8 < knn: all 8 are every point's neighbours; the oracle's value)
LONE_N = 32


def lone_cloud():
    """32 scattered points: one alone has the largest density (generator seed 92; with 91 and 94
    three points share their ten neighbours, and so the largest density)."""
    return np.random.default_rng(92).uniform(-1, 1, (LONE_N, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def lone_case():
    """MaxDensity where one point alone is saturated: maxDensity a quarter of the largest density,
    and the seed the first whose draw for that point lies in [accept (1 - 1/n), accept): the integer
    saturation factor (1) keeps it, the float factor (1 - 1/32) drops it. Chosen with the oracle's
    densities on the CPU."""
    import pyoracle as po

    pts = lone_cloud()
    dens = po.surface_normals(pts, 10)[1]
    top = int(np.argmax(dens))
    assert int(np.sum(dens == dens[top])) == 1
    md = f32(dens[top] / f32(4))
    accept = f32(md / dens[top])
    lo = f32(accept * f32(1.0 - 1.0 / LONE_N))
    for seed in range(1, 100000):
        r = uniform(seed, 4 * READING + 1, np.array([top]))[0]
        if lo <= r < accept:
            break
    return dict(pts=pts, side=READING, seed=seed, top=top,
                filters=[dict(kind=SN, knn=10, keep_densities=1), dict(kind=MAX_DENSITY, max_density=float(md))])


def _density_cases():
    sn = dict(kind=SN, knn=10, keep_densities=1)
    scattered = np.random.default_rng(97).uniform(-3, 3, (700, 3)).astype(f32)
    return {
        # a SurfaceNormal behind a dropping filter: its tree, its densities and the MaxDensity's draw
        # are those of the 587 points MinDist leaves (median density 3.04)
        "mindist_density": dict(pts=scattered, side=READING, seed=21,
                                filters=[dict(kind=MIN_DIST, dim=-1, min_dist=2.0), sn,
                                         dict(kind=MAX_DENSITY, max_density=3.0)]),
        # every point saturated: the integer factor is 0, every point is dropped
        "saturated_all": dict(pts=CUBE8, side=READING, seed=0, filters=[sn, dict(kind=MAX_DENSITY, max_density=1.0)],
                              want=np.zeros(8, bool)),
        # no point above maxDensity: nobody draws, all are kept (though all are saturated)
        "saturated_none_above": dict(pts=CUBE8, side=READING, seed=0,
                                     filters=[sn, dict(kind=MAX_DENSITY, max_density=50.0)], want=np.ones(8, bool)),
    }


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(pts, side, seed, filters[, want: the keep pattern known by construction])."""
    out = {}
    out.update(_compaction_cases())
    out.update(_axis_cases())
    out.update(_random_cases())
    out.update(_density_cases())
    out["saturated_lone"] = lone_case()
    return out


def has_densities(case):
    return any(f["kind"] == SN and f.get("keep_densities") for f in case["filters"])


def simulate(case, mut=None):
    """What Context.chain_filter would return if the device were this reference (with `mut` built in)."""
    r = run_filters(case["pts"], case["filters"], case["side"], case["seed"], None, mut)
    got = dict(n=len(r["index"]), counts=r["counts"], index=r["index"])
    if has_densities(case):
        import pyoracle as po

        sn = next(f for f in case["filters"] if f["kind"] == SN)
        got["densities"] = po.surface_normals(case["pts"][r["sn_index"]], sn["knn"])[1]
    return got


def _need(ok, msg):
    if not ok:
        raise Mismatch(msg)


def compare(case, got):
    """Device outputs of a case against the reference (run on the device's own densities)."""
    want = run_filters(case["pts"], case["filters"], case["side"], case["seed"], got.get("densities"))
    idx = np.asarray(got["index"])
    _need(got["n"] == len(want["index"]) == len(idx), f"kept {got['n']} ({len(idx)} indices) against {len(want['index'])}")
    _need(list(got["counts"]) == want["counts"], f"counts {got['counts']} against {want['counts']}")
    _need(bool(np.all(np.diff(idx) > 0)), "kept indices are not ascending")
    _need(np.array_equal(idx, want["index"]), "kept indices differ from the reference's")
    if "want" in case:
        _need(np.array_equal(idx, np.nonzero(case["want"])[0]), "kept indices differ from the pattern built in")


# ------------------------------------------------------------------ whole runs --------------
def plane_icp_reference(ref, read, ref_filters, read_filters, seed, knn=10, ratio=0.75, limit_d2=None, max_iter=100,
                        min_rot=1e-3, min_trans=1e-3, smooth=4, eps=0.0, bucket=8, dens_read=None, dens_ref=None,
                        margin=(2e-6, 2e-5), limit_margin=4e-5):
    """A whole point-to-plane run on a sampled chain, built as p2p_reference.icp_reference is: the
    filters above (with the device's densities where given), the normals of the full reference
    (pyoracle.surface_normals, the SurfaceNormal's position being first in the list) taken at the kept
    indices, pyoracle.Tree over the centred survivors, step_reference's point-to-plane sums and
    update, and pyoracle.dists_quantile (TrimmedDist) or the constant limit_d2 (MaxDist).
    MarginError: a smoothed cv0 / cv1 within `margin` of its threshold (as icp_reference), and under
    MaxDist a reading whose distance lies within limit_margin (m) of the limit's, where the device's
    transform (within the parity bar of this loop's) may put it on the other side.
    Returns dict(T, iterations, converged, status, kept, n_ref, n_read, index_ref, index_read)."""
    import pyoracle as po

    ref = np.ascontiguousarray(ref, f32)[:, :3]
    read = np.ascontiguousarray(read, f32)[:, :3]
    fr = run_filters(ref, ref_filters, REFERENCE, seed, dens_ref)
    fd = run_filters(read, read_filters, READING, seed, dens_read)
    assert fr["sn_n"] == len(ref), "the reference's SurfaceNormal comes first"
    nrm_full = po.surface_normals(ref, knn)[0]
    refF, nrm, rdF = ref[fr["index"]], nrm_full[fr["index"]], read[fd["index"]]
    mean = np.array([pr._fixed40_mean(refF[:, d]) for d in range(3)], f32)
    refc = (refF - mean).astype(f32)
    tree = po.Tree(refc, bucket)
    Tmean = sr.ident16()
    Tmean[12:15] = mean
    TrmDin = sr.ident16()
    TrmDin[12:15] = -mean
    rd = sr.apply_points(TrmDin, rdF)
    prm = dict(max_iter=max_iter, smooth=smooth, min_rot=min_rot, min_trans=min_trans)
    st = sr.State()
    out = dict(kept=[], cv=[], n_ref=len(refF), n_read=len(rdF), index_ref=fr["index"], index_read=fd["index"])
    n = len(rd)
    while st.active:
        step = sr.apply_points(st.T, rd)
        ids, d2, _, _ = tree.knn(step, 1, eps)
        ids, d2 = ids[:, 0], d2[:, 0]
        if limit_d2 is None:
            limit, qerr = po.dists_quantile(d2, ratio)
            if qerr:
                st.status, st.active = 1, 0
                break
        else:
            limit = f32(limit_d2)
            with np.errstate(invalid="ignore"):
                near = np.abs(np.sqrt(d2.astype(f64)) - math.sqrt(float(limit))) < limit_margin
            if near.any():
                raise MarginError(f"iteration {st.iters}: {int(near.sum())} distances within {limit_margin} of the limit")
        with np.errstate(invalid="ignore"):
            idx = np.nonzero(d2 <= f32(limit))[0]
        F, dot = sr.terms(st.T, rd[idx], refc[ids[idx]], nrm[ids[idx]])
        prod = sr.products(F, dot)
        tot = np.zeros(sr.COLS)
        tot[:27] = [math.fsum(prod[:, c].tolist()) for c in range(27)]
        tot[27] = len(idx)
        u = sr.update(st, tot, n, prm)
        out["kept"].append(len(idx))
        out["cv"].append((u["cv0"], u["cv1"]))
        if u["cv0"] is not None:
            for cv, thr, mg, what in ((u["cv0"], float(f32(min_rot)), margin[0], "cv0"),
                                      (u["cv1"], float(f32(min_trans)), margin[1], "cv1")):
                if abs(cv - thr) < mg:
                    raise MarginError(f"iteration {st.iters}: {what} {cv!r} within {mg} of {thr!r}")
    T = sr.mul4(sr.mul4(Tmean, st.T), TrmDin)
    status = st.status
    if status == 0 and not sr.rigid_ok(T):
        status = 5
    out.update(T=T.reshape(4, 4).T.copy(), iterations=st.iters, converged=st.converged, status=status)
    return out
