"""The batch form of the sampled chains' filters: one side's list over several clouds
at once. The reference of test_chain_batch_cpu.py and test_chain_batch.py.

The expected result of a ragged batch is chain_reference.run_filters applied cloud by cloud
(expected()). simulate() restates what the device does instead: the clouds laid end to end, one
keep flag per row of the concatenation, the kept rows compacted in order, and every cloud's next
count and offset taken from the ranks at its two ends. Unmutated it equals expected(); with one of
MUTATIONS built in it goes wrong the way the batch form can and the one-pair form cannot:

  concat_index   the draw indexed by the row's position in the concatenation, not in its own cloud
  side_max       MaxDensity's maximum and saturated count taken over the whole side
  straddle       a 64-row wave that straddles two clouds credited wholly to the cloud of its first row
  empty_shift    an emptied cloud taking one row of the offsets of the clouds behind it
  reading_slot   a reference filtered under the reading side's slot of the draw

CASES are the batches the GPU tests run.
"""
import functools

import numpy as np

import chain_reference as cr
from chain_reference import MAX_DENSITY, MIN_DIST, RANDOM, READING, REFERENCE, SN, f32

MUTATIONS = ("concat_index", "side_max", "straddle", "empty_shift", "reading_slot")
WAVE = 64
# 63 + 1: a boundary inside the first wave and one on its edge; 65: inside the third wave; 1023 ends at
# row 1152, inside the second 1024-row tile; 1025 at 2177, inside the third; 4097 spans four tiles
RAGGED = (63, 1, 65, 1023, 1025, 4097)


# ------------------------------------------------------------------ the cases ---------------
def _scatter(n, seed, half=6.0):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(f32)


def _ragged_cases():
    out = {}
    clouds = [_scatter(n, 300 + k) for k, n in enumerate(RAGGED)]
    out["ragged_random"] = dict(clouds=clouds, side=READING, seed=11, filters=[dict(kind=RANDOM, prob=0.5)])
    out["ragged_random_ref"] = dict(clouds=clouds[::-1], side=REFERENCE, seed=12345, filters=[dict(kind=RANDOM, prob=0.3)])
    # points exactly on the radius (chain_reference.RADIUS's construction), every second point kept
    pat = [cr._pattern_cloud(n, np.arange(n) % 2 == 0) for n in RAGGED]
    out["ragged_radius"] = dict(clouds=pat, side=READING, seed=0, filters=[dict(kind=MIN_DIST, dim=-1, min_dist=cr.RADIUS)],
                                want=[np.arange(n) % 2 == 0 for n in RAGGED])
    # a cloud in the middle that MinDist empties (every point on the radius or inside it), then a
    # draw whose index is the position after MinDist in the point's own cloud
    mid = [pat[0], pat[3], cr._pattern_cloud(65, np.zeros(65, bool)), pat[4], cr._pattern_cloud(1, np.zeros(1, bool)),
           pat[2]]
    out["emptied_middle"] = dict(clouds=mid, side=REFERENCE, seed=3,
                                 filters=[dict(kind=MIN_DIST, dim=-1, min_dist=cr.RADIUS), dict(kind=RANDOM, prob=0.5)])
    return out


def _density_cases():
    sn = dict(kind=SN, knn=10, keep_densities=1)
    # densities with different maxima; the cube's points are all saturated (2.94 each), and above
    # maxDensity 1: the integer factor drops every one of them, which empties the cloud
    clouds = [_scatter(700, 97, 3.0), cr.CUBE8, cr.lone_cloud(), _scatter(300, 98, 1.5), _scatter(129, 99, 2.0)]
    out = {
        "density_maxima": dict(clouds=clouds, side=READING, seed=21, filters=[sn, dict(kind=MAX_DENSITY, max_density=1.0)]),
        # a SurfaceNormal behind a dropping filter that empties a cloud in the middle: its trees, its
        # densities and the MaxDensity's draw are those of what MinDist leaves of each cloud
        "mindist_density": dict(clouds=[_scatter(700, 97, 3.0), _scatter(40, 5, 0.5), _scatter(300, 96, 3.0)], side=READING,
                                seed=21, filters=[dict(kind=MIN_DIST, dim=-1, min_dist=2.0), sn,
                                                  dict(kind=MAX_DENSITY, max_density=3.0)]),
        # the reference's shape: normals carried through a sampling
        "normals_random": dict(clouds=[_scatter(257, 90, 2.0), _scatter(5, 91, 1.0), _scatter(1100, 92, 3.0)],
                               side=REFERENCE, seed=7, filters=[dict(kind=SN, knn=10, keep_densities=0),
                                                                dict(kind=RANDOM, prob=0.5)]),
    }
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(clouds, side, seed, filters[, want: per cloud the keep pattern known by construction])."""
    out = {}
    out.update(_ragged_cases())
    out.update(_density_cases())
    return out


def has_densities(case):
    return cr.has_densities(case)


def has_normals(case):
    return any(f["kind"] == SN and f["knn"] in (10, 20, 30) for f in case["filters"])


# ------------------------------------------------------------------ the expected result -----
def oracle_densities(case):
    """Per cloud, the oracle's densities of the cloud as the SurfaceNormal receives it (None without one)."""
    if not has_densities(case):
        return [None] * len(case["clouds"])
    import pyoracle as po

    sn = next(q for q, f in enumerate(case["filters"]) if f["kind"] == SN)
    out = []
    for c in case["clouds"]:
        idx = cr.run_filters(c, case["filters"][:sn], case["side"], case["seed"])["index"]
        out.append(po.surface_normals(np.ascontiguousarray(c[idx], f32), case["filters"][sn]["knn"])[1] if len(idx)
                   else np.zeros(0, f32))
    return out


def expected(case, densities=None):
    """chain_reference.run_filters cloud by cloud. densities: per cloud, at the SurfaceNormal (the
    device's own in the GPU tests; None: the oracle's)."""
    dens = densities if densities is not None else oracle_densities(case)
    out = []
    fl = case["filters"]
    for c, d in zip(case["clouds"], dens):
        r = None
        for k, f in enumerate(fl):
            # (run_filters' MaxDensity takes a cloud with a point: an emptied one stays empty)
            if f["kind"] == MAX_DENSITY:
                head = cr.run_filters(c, fl[:k], case["side"], case["seed"], d)
                if len(head["index"]) == 0:
                    r = dict(index=head["index"], counts=head["counts"] + [0] * (len(fl) - k))
                    break
        if r is None:
            r = cr.run_filters(c, fl, case["side"], case["seed"], d)
        out.append(dict(n=len(r["index"]), counts=r["counts"], index=r["index"]))
    return out


# ------------------------------------------------------------------ the device, restated ----
def simulate(case, mut=None, densities=None):
    """What Context.test_chain_batch would return if the device were this restatement (with `mut`
    built in): per cloud dict(n, counts, index)."""
    assert mut is None or mut in MUTATIONS, mut
    clouds = [np.ascontiguousarray(c, f32)[:, :3] for c in case["clouds"]]
    C = len(clouds)
    side = case["side"]
    # the concatenation: each row's cloud and index in its own cloud as given
    rows = np.concatenate([np.arange(len(c)) for c in clouds])
    n = np.array([len(c) for c in clouds])
    off = np.r_[0, np.cumsum(n)[:-1]]
    dens = None
    counts = [[] for _ in range(C)]
    for pos, f in enumerate(case["filters"]):
        slot_side = READING if (mut == "reading_slot" and side == REFERENCE) else side
        slot = 4 * slot_side + pos
        kind = f["kind"]
        total = int(n.sum())
        keep = np.ones(total, bool)
        if kind == SN:
            if f.get("keep_densities"):
                if densities is not None:
                    dens_in = [np.asarray(d, f32) for d in densities]
                else:   # the oracle's, of each cloud as it stands here
                    import pyoracle as po

                    dens_in = [po.surface_normals(np.ascontiguousarray(clouds[c][rows[off[c]:off[c] + n[c]]], f32),
                                                  f["knn"])[1] if n[c] else np.zeros(0, f32) for c in range(C)]
                dens = np.concatenate(dens_in) if total else np.zeros(0, f32)
                assert len(dens) == total, (len(dens), total)
        else:
            with np.errstate(all="ignore"):
                side_last = f32(dens.max()) if (kind == MAX_DENSITY and total) else None
                for c in range(C):
                    sl = slice(off[c], off[c] + n[c])
                    if n[c] == 0:
                        continue
                    i = np.arange(n[c]) + (off[c] if mut == "concat_index" else 0)
                    if kind == MIN_DIST:
                        keep[sl] = cr.min_dist_keep(clouds[c][rows[sl]], f.get("dim", -1), f.get("min_dist", 1.0))
                    elif kind == RANDOM:
                        keep[sl] = cr.uniform(case["seed"], slot, i) < f32(f.get("prob", 0.75))
                    elif kind == MAX_DENSITY:
                        d = dens[sl]
                        md = f32(f.get("max_density", 10.0))
                        if mut == "side_max":
                            last, n_sat, n_in = side_last, int(np.sum(dens == side_last)), total
                        else:
                            last, n_sat, n_in = f32(d.max()), int(np.sum(d == d.max())), int(n[c])
                        accept = (md / d).astype(f32)
                        accept = np.where(d == last, (accept * f32(1 - n_sat // n_in)).astype(f32), accept)
                        keep[sl] = ~(d > md) | (cr.uniform(case["seed"], slot, i) < accept)
                    else:
                        raise ValueError(kind)
        # the compaction of the whole concatenation, in order
        kept_rows = rows[keep]
        kept_dens = dens[keep] if dens is not None else None
        rank = np.r_[0, np.cumsum(keep)]       # kept rows before row b
        if mut == "straddle" and kind != SN:
            # every wave's kept count to the cloud that holds the wave's first row
            cloud_of = np.repeat(np.arange(C), n)
            n2 = np.zeros(C, int)
            for w0 in range(0, total, WAVE):
                n2[cloud_of[w0]] += int(keep[w0:w0 + WAVE].sum())
        else:
            n2 = np.array([rank[off[c] + n[c]] - rank[off[c]] for c in range(C)], int)
        off2 = np.r_[0, np.cumsum(n2)[:-1]].astype(int)
        if mut == "empty_shift":
            emptied = (n > 0) & (n2 == 0)
            off2 = off2 + np.r_[0, np.cumsum(emptied)[:-1]]
        # each cloud's rows as the next stage finds them at its offset
        pad = np.r_[kept_rows, np.zeros(C + 1, kept_rows.dtype)]
        new_rows = [pad[off2[c]:off2[c] + n2[c]] for c in range(C)]
        if kept_dens is not None:
            padd = np.r_[kept_dens, np.zeros(C + 1, f32)]
            dens = np.concatenate([padd[off2[c]:off2[c] + n2[c]] for c in range(C)]) if n2.sum() else np.zeros(0, f32)
        rows = np.concatenate(new_rows) if n2.sum() else np.zeros(0, int)
        n = n2
        off = np.r_[0, np.cumsum(n)[:-1]].astype(int)
        for c in range(C):
            counts[c].append(int(n[c]))
    return [dict(n=int(n[c]), counts=counts[c], index=rows[off[c]:off[c] + n[c]].astype(np.int32)) for c in range(C)]


def mismatches(case, got, densities=None):
    """The clouds of `got` (test_chain_batch's shape) that differ from expected(): a list of messages."""
    want = expected(case, densities)
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} clouds against {len(want)}"]
    for c, (g, w) in enumerate(zip(got, want)):
        if g["n"] != w["n"] or list(g["counts"]) != list(w["counts"]):
            bad.append(f"cloud {c}: kept {g['n']} counts {list(g['counts'])} against {w['n']} {w['counts']}")
        elif not np.array_equal(np.asarray(g["index"]), w["index"]):
            bad.append(f"cloud {c}: kept indices differ")
        elif "want" in case and not np.array_equal(np.asarray(g["index"]), np.nonzero(case["want"][c])[0]):
            bad.append(f"cloud {c}: kept indices differ from the pattern built in")
    return bad
