"""Plain-numpy restatement of the tail of a point-to-point ICP iteration, k_icp_reduce_p2p +
k_icp_update_p2p: the reference of test_p2p_step_kernels.py (Context.test_step_p2p /
aicp_hip_test_step_p2p), and of whole point-to-point runs (icp_reference, test_p2p_registration.py).

Terms. p = T r in float32, one rounded operation at a time in apply4's order (the library is built
with -ffp-contract=off, so these are the device's floats); q the matched reference point. A slab row
holds, over the row's kept readings (d2 <= limit): columns 0..8 sum q_a p_b (index 3a + b; a product
of two floats is exact in double), 9..11 sum p, 12..14 sum q (the floats themselves), 15..26 +0.0,
27 kept, 28 / 29 touched points / nodes.

Sums. As step_reference: each of the 15 floating columns of a row, and of a pair's total, within
(n + 2) 2^-53 sum|t_i| of math.fsum of its exact terms, n the kept count; columns 15..26 exactly
+0.0; 27..29 exact integers; rows of an inactive pair hold the sentinel.

Update, bit for bit. From the device's own rows: the totals in k_icp_update_p2p's order (group g
sums rows g, g + 8, ... in order, then the 8 groups in order), then update_serial_p2p restated in
numpy scalars of the same widths: pm = sum p / n, qm = sum q / n, M = S - (sum q)(sum p)^T / n,
svd3 (one-sided Jacobi: only + - * / sqrt, so the restatement is exact), the rank rule
(sig_i > sig_0 * 3 FLT_EPSILON), R = U V^T with the determinant rule, the cross products at rank 2,
R = I below rank 2, t = qm - R pm, one rounding to float, mul4, and the checkers' tail shared with
the point-to-plane update. T_iter, kept, iters, status, active, converged, hist_count, inlier_ratio,
the touch totals and dt must equal the device's exactly, dq within 4 ulp (atan2). MarginError as in
step_reference: the smoothed cv0 / cv1 within 1e-9 relative of min_rot / min_trans.

simulate() makes "device outputs" from the reference itself (optionally with one of MUTATIONS built
in), compare() checks device outputs; CASES is the table of inputs the GPU tests run.
"""
import functools
import math

import numpy as np

import step_reference as sr
from step_reference import (COLS, DQ, DT, GROUPS, QH, RB, RING, SENTINEL_BITS, TH, U, MarginError, Mismatch,
                            State, _need, _same_floats, apply_points, f32, f64, layout, mul4, params, rigid_ok,
                            ulp_diff, INT_KEYS)

FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = f64(np.finfo(np.float64).eps)
SWEEPS = 30        # kSvd3Sweeps
NF = 15            # floating columns of a row
MUTATIONS = ("lt", "drop_tail", "ref_off", "transposeM", "no_det_fix", "no_means", "rows128")


# ------------------------------------------------------------------ the 3x3 SVD ------------
def _sqrt(x):
    return f64(math.sqrt(x)) if x >= 0 else f64(np.nan)


def svd3(M):
    """icp_math.hpp svd3 in numpy float64 scalars. M: 3x3 (row-major nested or array).
    Returns U, sig, V as lists (U, V: 3 rows of 3)."""
    with np.errstate(all="ignore"):
        a = [[f64(M[r][c]) for c in range(3)] for r in range(3)]
        V = [[f64(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
        one, two = f64(1.0), f64(2.0)
        for _ in range(SWEEPS):
            rotated = False
            for p, q in ((0, 1), (0, 2), (1, 2)):
                al = (a[0][p] * a[0][p] + a[1][p] * a[1][p]) + a[2][p] * a[2][p]
                be = (a[0][q] * a[0][q] + a[1][q] * a[1][q]) + a[2][q] * a[2][q]
                ga = (a[0][p] * a[0][q] + a[1][p] * a[1][q]) + a[2][p] * a[2][q]
                if ga * ga > (DBL_EPS * DBL_EPS) * (al * be):
                    rotated = True
                    ze = (be - al) / (two * ga)
                    az = -ze if ze < 0 else ze
                    tt = (f64(-1.0) if ze < 0 else one) / (az + _sqrt(ze * ze + one))
                    cc = one / _sqrt(tt * tt + one)
                    ss = tt * cc
                    for k in range(3):
                        ap, aq = a[k][p], a[k][q]
                        a[k][p] = cc * ap - ss * aq
                        a[k][q] = ss * ap + cc * aq
                        vp, vq = V[k][p], V[k][q]
                        V[k][p] = cc * vp - ss * vq
                        V[k][q] = ss * vp + cc * vq
            if not rotated:
                break
        sig = [_sqrt((a[0][j] * a[0][j] + a[1][j] * a[1][j]) + a[2][j] * a[2][j]) for j in range(3)]
        for j in (0, 1, 0):
            if sig[j] < sig[j + 1]:
                sig[j], sig[j + 1] = sig[j + 1], sig[j]
                for k in range(3):
                    a[k][j], a[k][j + 1] = a[k][j + 1], a[k][j]
                    V[k][j], V[k][j + 1] = V[k][j + 1], V[k][j]
        Um = [[a[k][j] / sig[j] if sig[j] > 0 else a[k][j] for j in range(3)] for k in range(3)]
    return Um, sig, V


def det3(R):
    d0 = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1])
    d1 = R[1][0] * (R[0][1] * R[2][2] - R[0][2] * R[2][1])
    d2 = R[2][0] * (R[0][1] * R[1][2] - R[0][2] * R[1][1])
    return (d0 - d1) + d2


def p2p_rotation(M, mut=None):
    """icp_math.hpp p2p_rotation: (R as 3 rows of 3 float64, rank)."""
    with np.errstate(all="ignore"):
        Um, sig, V = svd3(M)
        thr = sig[0] * f64(3.0 * FLT_EPS)
        rank = sum(1 for j in range(3) if sig[j] > thr)
        if rank < 2:
            return [[f64(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)], rank
        if rank == 2:
            for X in (Um, V):
                X[0][2] = X[1][0] * X[2][1] - X[2][0] * X[1][1]
                X[1][2] = X[2][0] * X[0][1] - X[0][0] * X[2][1]
                X[2][2] = X[0][0] * X[1][1] - X[1][0] * X[0][1]
        R = [[(Um[r][0] * V[c][0] + Um[r][1] * V[c][1]) + Um[r][2] * V[c][2] for c in range(3)] for r in range(3)]
        if rank == 3 and det3(R) < 0 and mut != "no_det_fix":
            R = [[(Um[r][0] * V[c][0] + Um[r][1] * V[c][1]) - Um[r][2] * V[c][2] for c in range(3)]
                 for r in range(3)]
    return R, rank


def cross_covariance(tot, mut=None):
    """pm, qm, M of update_serial_p2p from a pair's totals."""
    with np.errstate(all="ignore"):
        n = f64(int(tot[27]))
        sp = [f64(tot[9 + a]) for a in range(3)]
        sq = [f64(tot[12 + a]) for a in range(3)]
        pm = [sp[a] / n for a in range(3)]
        qm = [sq[a] / n for a in range(3)]
        if mut == "no_means":
            M = [[f64(tot[3 * a + b]) for b in range(3)] for a in range(3)]
        else:
            M = [[f64(tot[3 * a + b]) - (sq[a] * sp[b]) / n for b in range(3)] for a in range(3)]
        if mut == "transposeM":
            M = [[M[b][a] for b in range(3)] for a in range(3)]
    return pm, qm, M


def delta_from_totals(tot, mut=None):
    """dT (16 float32, column-major) and the rank, from a pair's totals."""
    with np.errstate(all="ignore"):
        pm, qm, M = cross_covariance(tot, mut)
        R, rank = p2p_rotation(M, mut)
        dT = np.zeros(16, f32)
        for a in range(3):
            t = qm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])
            for b in range(3):
                dT[b * 4 + a] = f32(R[a][b])
            dT[12 + a] = f32(t)
        dT[15] = 1
    return dT, rank


def checkers_tail(st, kept, n_read, prm):
    """update_tail (kernels_icp.hip): the inlier ratio and the checkers, after T_iter's composition.
    Returns (cv0, cv1), None where not reached."""
    cvs = (None, None)
    ix = lambda h: h % RING
    st.inlier_ratio = f32(f64(f32(kept)) / f64(n_read))
    if not rigid_ok(st.T):
        st.iters += 1
        st.status, st.active = 5, 0
        return cvs
    iterate = True
    st.iters += 1
    if st.iters >= prm["max_iter"]:
        iterate = False
    R = st.ring
    h = ix(st.hist_count)
    R[QH + 4 * h:QH + 4 * h + 4] = sr.quat_from_T(st.T)
    R[TH + 3 * h:TH + 3 * h + 3] = [f64(st.T[12 + i]) for i in range(3)]
    if st.hist_count >= 1:
        bp = ix(st.hist_count - 1)
        R[DQ + h] = abs(sr.quat_angdist(R[QH + 4 * h:QH + 4 * h + 4], R[QH + 4 * bp:QH + 4 * bp + 4]))
        d = R[TH + 3 * h:TH + 3 * h + 3] - R[TH + 3 * bp:TH + 3 * bp + 3]
        R[DT + h] = sr._sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    st.hist_count += 1
    sz = st.hist_count
    if sz > prm["smooth"]:
        cv0 = cv1 = f64(0)
        for i in range(sz - 1, sz - prm["smooth"] - 1, -1):
            cv0 = cv0 + R[DQ + ix(i)]
            cv1 = cv1 + R[DT + ix(i)]
        cv0 = cv0 / prm["smooth"]
        cv1 = cv1 / prm["smooth"]
        cvs = (float(cv0), float(cv1))
        if cv0 != cv0 or cv1 != cv1:
            st.status, st.active = 1, 0
            return cvs
        mr, mt = float(f32(prm["min_rot"])), float(f32(prm["min_trans"]))
        for cv, thr, what in ((cv0, mr, "cv0 against min_rot"), (cv1, mt, "cv1 against min_trans")):
            if thr > 0 and abs(float(cv) - thr) < 1e-9 * thr:
                raise MarginError(f"{what}: {float(cv)!r} within 1e-9 of {thr!r}")
        if cv0 < mr and cv1 < mt:
            if iterate:
                st.converged = 1
            iterate = False
    st.active = 1 if iterate else 0
    return cvs


def update(st, tot, n_read, prm, mut=None):
    """update_serial_p2p on the sums tot; returns dict(rank, cv0, cv1) (None where not reached)."""
    info = dict(rank=None, cv0=None, cv1=None)
    with np.errstate(all="ignore"):
        st.touched_pts += int(tot[28])
        st.touched_nodes += int(tot[29])
        kept = int(tot[27])
        st.kept = kept
        if kept == 0:
            st.status, st.active = 1, 0
            return info
        dT, info["rank"] = delta_from_totals(tot, mut)
        st.T = mul4(dT, st.T)
        info["cv0"], info["cv1"] = checkers_tail(st, kept, n_read, prm)
    return info


# ------------------------------------------------------------------ a case's terms ---------
def products(p, q):
    """(k, 15) exact doubles: q_a p_b (3a + b), then p, then q."""
    with np.errstate(all="ignore"):
        p = p.astype(f64)
        q = q.astype(f64)
        cols = [q[:, a] * p[:, b] for a in range(3) for b in range(3)] + [p[:, a] for a in range(3)] + \
               [q[:, a] for a in range(3)]
    return np.stack(cols, axis=1) if len(p) else np.zeros((0, NF))


def pair_terms(case, s, p, T, limit, mut=None):
    """The kept readings of pair p in step s: their indices, exact terms (k, 15), and the touch
    counts of every reading the reduce reads."""
    n_read, offs, _, _ = layout(case)
    o, n = int(offs[p]), int(n_read[p])
    d2 = np.asarray(case["d2"], f32)[s, o:o + n]
    match = np.asarray(case["match"], np.int32)[s, o:o + n]
    tc = np.asarray(case["touched"], np.uint32)[s, o:o + n].astype(np.uint64)
    with np.errstate(invalid="ignore"):
        keep = d2 < f32(limit) if mut == "lt" else d2 <= f32(limit)
    read = np.ones(n, bool)
    if mut == "drop_tail" and n % RB:
        read[n - 1] = False
    keep &= read
    idx = np.nonzero(keep)[0]
    ref_pts = np.asarray(case["ref_pts"], f32).reshape(-1, 3)
    g = int(case["ref_off"][p]) + (1 if mut == "ref_off" and p == 1 else 0) + match[idx].astype(np.int64)
    g = np.minimum(g, ref_pts.shape[0] - 1)
    r = np.asarray(case["read_c"], f32).reshape(-1, 3)[o + idx]
    pp = apply_points(np.asarray(T, f32), r)
    return idx, products(pp, ref_pts[g]), (tc & 0xFFFF) * read, (tc >> 16) * read


def total_from_rows(rows, mut=None):
    return sr.total_from_rows(rows, mut)


def own_rows(idx, prod, tp, tn, nrow):
    rows = np.zeros((nrow, COLS))
    with np.errstate(all="ignore"):
        for r in range(nrow):
            sel = (idx // RB) == r
            rows[r, :NF] = prod[sel].sum(axis=0)
            rows[r, 27] = int(sel.sum())
            rows[r, 28] = int(tp[r * RB:(r + 1) * RB].sum())
            rows[r, 29] = int(tn[r * RB:(r + 1) * RB].sum())
    return rows


def _zero_columns(block, what):
    z = np.ascontiguousarray(block[..., NF:27]).view(np.uint64)
    _need(bool(np.all(z == 0)), f"{what}: columns 15..26 are not +0.0")


def check_slab(dev_rows, idx, prod, tp, tn, what, mut=None):
    """A pair's device rows, and their total in the update's order, against the exact sums."""
    nrow = dev_rows.shape[0]
    rid = idx // RB
    _zero_columns(dev_rows, what)
    for r in range(nrow):
        sel = rid == r
        k = int(sel.sum())
        want = (k, int(tp[r * RB:(r + 1) * RB].sum()), int(tn[r * RB:(r + 1) * RB].sum()))
        got = tuple(dev_rows[r, 27:])
        _need(got == tuple(float(v) for v in want), f"{what} row {r}: kept / touched {got} against {want}")
        for c in range(NF):
            sr._check_sum(float(dev_rows[r, c]), prod[sel, c], k, f"{what} row {r} column {c}")
    tot = total_from_rows(dev_rows, mut)
    want = (len(idx), int(tp.sum()), int(tn.sum()))
    _need(tuple(tot[27:]) == tuple(float(v) for v in want),
          f"{what} totals: kept / touched {tuple(tot[27:])} against {want}")
    for c in range(NF):
        sr._check_sum(float(tot[c]), prod[:, c], len(idx), f"{what} total column {c}")
    return tot


def simulate(case, mut=None):
    """What Context.test_step_p2p would return if the device were this reference (with `mut` built in)."""
    n_read, _, nrow, roff = layout(case)
    prm = params(case)
    out = sr._empty(case)
    out["slab"].view(np.uint64)[:] = SENTINEL_BITS
    states = sr.initial_states(case)
    S, P = out["kept"].shape
    for s in range(S):
        for p, st in enumerate(states):
            if st.active:
                st.limit = f32(np.asarray(case["limit"], f32)[s, p])
                idx, prod, tp, tn = pair_terms(case, s, p, st.T, st.limit, mut)
                rows = own_rows(idx, prod, tp, tn, int(nrow[p]))
                out["slab"][s, roff[p]:roff[p + 1]] = rows
                update(st, total_from_rows(rows, mut), int(n_read[p]), prm, mut)
            sr._record(out, s, p, st)
    return out


def compare(case, got):
    """Device outputs against the reference; raises Mismatch. Returns dict(max_dq_ulp, ranks, cv):
    ranks[s][p] the rank of M on the device's totals (None: no update), cv[s][p] the smoothed
    (cv0, cv1)."""
    n_read, _, nrow, roff = layout(case)
    prm = params(case)
    want = sr._empty(case)
    states = sr.initial_states(case)
    S, P = want["kept"].shape
    _need(got["slab"].shape == want["slab"].shape, "slab shape")
    info = dict(max_dq_ulp=0, ranks=[], cv=[])
    for s in range(S):
        info["ranks"].append([None] * P)
        info["cv"].append([None] * P)
        for p, st in enumerate(states):
            dev = got["slab"][s, roff[p]:roff[p + 1]]
            what = f"step {s} pair {p}"
            if st.active:
                st.limit = f32(np.asarray(case["limit"], f32)[s, p])
                idx, prod, tp, tn = pair_terms(case, s, p, st.T, st.limit)
                tot = check_slab(dev, idx, prod, tp, tn, what)
                u = update(st, tot, int(n_read[p]), prm)
                info["ranks"][s][p] = u["rank"]
                info["cv"][s][p] = (u["cv0"], u["cv1"])
            else:
                _need(bool(np.all(np.ascontiguousarray(dev).view(np.uint64) == SENTINEL_BITS)),
                      f"{what}: an inactive pair's rows were written")
            sr._record(want, s, p, st)
            _need(_same_floats(got["T"][s, p], want["T"][s, p]),
                  f"{what}: T_iter {got['T'][s, p]} against {want['T'][s, p]}")
            for k in INT_KEYS + ("touched_pts", "touched_nodes"):
                _need(int(got[k][s, p]) == int(want[k][s, p]), f"{what}: {k} {got[k][s, p]} against {want[k][s, p]}")
            _need(_same_floats(got["inlier_ratio"][s, p], want["inlier_ratio"][s, p]), f"{what}: inlier_ratio")
            _need(_same_floats(got["dt"][s, p], want["dt"][s, p]),
                  f"{what}: dt {got['dt'][s, p]!r} against {want['dt'][s, p]!r}")
            d = ulp_diff(got["dq"][s, p], want["dq"][s, p])
            info["max_dq_ulp"] = max(info["max_dq_ulp"], d)
            _need(d <= 4, f"{what}: dq {got['dq'][s, p]!r} against {want['dq'][s, p]!r}: {d} ulp")
    _need(got["dirty"] == 0, f"{got['dirty']} arrival counters left non-zero")
    return info


# ------------------------------------------------------------------ the cases ---------------
# step_reference's inputs serve where the normals play no part (they are not read): the tails on
# both sides of a block and of a row with none / half / all kept, the ties and non-finite distances,
# the ragged six-pair batch, the 129-row pair, statuses 1 and 5.
TAILS = (1, 255, 257, 1023, 1025)
SHARED = tuple(f"tail{n}" for n in TAILS) + ("ties", "ragged", "rows129", "none_kept", "nonrigid")


def rot(axis, angle):
    """Rodrigues rotation matrix (3x3 double)."""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _pair_from(rng, q, r, match, keep=None):
    """A pair whose kept readings (d2 0.25 against limit 0.5; the others 1.0) are `keep` (all by default)."""
    n = len(r)
    keep = np.ones(n, bool) if keep is None else keep
    d2 = np.where(keep, f32(0.25), f32(1.0)).astype(f32)
    touched = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return dict(q=q.astype(f32), nrm=np.zeros((len(q), 3), f32), r=r.astype(f32), match=match.astype(np.int32),
                d2=d2, touched=touched, limit=f32(0.5))


def _moved(rng, q, match, Rm, t, noise=0.0):
    """Readings that Rm, t map onto their matches (plus noise)."""
    tgt = q[match].astype(f64) + noise * rng.normal(size=(len(match), 3))
    return (tgt - t) @ Rm   # = Rm^T (tgt - t) per row


def case_exact():
    """The reading is a subset of the reference moved by a known rigid transform, ratio 1: one step
    returns that transform (EXACT_R, EXACT_T)."""
    rng = np.random.default_rng(51)
    q = rng.uniform(-5, 5, (400, 3)).astype(f32)
    match = rng.permutation(400)[:300]
    r = _moved(rng, q, match, EXACT_R, EXACT_T)
    return sr._batch([_pair_from(rng, q, r, match)])


EXACT_R, EXACT_T = rot((0.3, -0.5, 0.8), 0.4), np.array([0.7, -0.3, 0.25])


def _planar(rng, n, zamp):
    q = rng.uniform(-5, 5, (n, 3))
    q[:, 2] = zamp * rng.uniform(-1, 1, n)
    return q.astype(f32)


def case_reflection():
    """A mirrored planar patch: q = (x, y, z), r = (x, y, -z) with |z| <= 0.05 against 5 m extents.
    M is diag(+, +, -) up to noise: the unconstrained optimum is a reflection, det(U V^T) = -1, and
    the determinant rule returns a proper rotation (near the identity). Two steps."""
    rng = np.random.default_rng(53)
    q = _planar(rng, 300, 0.05)
    r = q.copy()
    r[:, 2] = -r[:, 2]
    pr = _pair_from(rng, q, r, np.arange(300))
    return sr._batch([pr], n_steps=2)


def case_p2p_ranks():
    """Four pairs whose M has rank 3, 2, 1 and 0 on exact data: a general scene; an exactly planar
    patch (z = 0) rotated in its plane; collinear points shifted along x; a single kept reading. Two
    steps."""
    rng = np.random.default_rng(57)
    pairs = []
    q = rng.uniform(-5, 5, (200, 3)).astype(f32)
    m = rng.integers(0, 200, 700)
    pairs.append(_pair_from(rng, q, _moved(rng, q, m, rot((1, 2, 3), 0.05), np.array([0.1, 0.0, -0.1]), 0.01), m,
                            rng.random(700) < 0.5))
    q = _planar(rng, 200, 0.0)
    m = rng.integers(0, 200, 700)
    pairs.append(_pair_from(rng, q, _moved(rng, q, m, rot((0, 0, 1), 0.05), np.array([0.1, -0.2, 0.0])), m,
                            rng.random(700) < 0.5))
    s = rng.uniform(-5, 5, 200)
    q = np.stack([s, 2 * s, -s], axis=1).astype(f32)
    m = rng.integers(0, 200, 700)
    pairs.append(_pair_from(rng, q, q[m].astype(f64) + np.array([0.1, 0.0, 0.0]), m, rng.random(700) < 0.5))
    q = rng.uniform(-5, 5, (200, 3)).astype(f32)
    m = rng.integers(0, 200, 700)
    one = np.zeros(700, bool)
    one[333] = True
    pairs.append(_pair_from(rng, q, q[m].astype(f64) + 0.02 * rng.normal(size=(700, 3)), m, one))
    return sr._batch(pairs, n_steps=2)


RANKS = (3, 2, 1, 0)
# z amplitudes of a planar patch of 5 m half-extent: sig_2 / sig_0 is about (z / 5)^2, and the rank
# threshold 3 FLT_EPSILON = 3.6e-7 lies at z of about 3e-3
THRESHOLD_Z = (1e-5, 1e-4, 1e-3) + tuple(float(10.0 ** (-2.9 + 0.1 * k)) for k in range(9)) + (1e-2, 1e-1)


def case_p2p_threshold():
    """A patch of z amplitude s, one pair per s in THRESHOLD_Z, turned about a tilted axis: M goes
    from rank 2 (cross products) to rank 3 (U V^T with the determinant test) in steps of 10^0.1
    across the threshold; two steps."""
    rng = np.random.default_rng(59)
    pairs = []
    for s in THRESHOLD_Z:
        q = _planar(rng, 64, s)
        m = rng.integers(0, 64, 500)
        pairs.append(_pair_from(rng, q, _moved(rng, q, m, rot((0.2, -0.1, 1), 0.03), np.array([0.05, 0.02, -0.01])),
                                m, rng.random(500) < 0.5))
    return sr._batch(pairs, n_steps=2)


RING_STEPS, RING_GROUP, RING_SHRINK = 40, 64, 0.8
RING_CONVERGES = 35
RING_SMOOTH = (1, 4, 31)


@functools.lru_cache(maxsize=None)
def _ring_base():
    """2560 readings in 40 groups of 64; step s keeps group s alone, whose readings lie at
    T_s^-1 dT_s^-1 q for the T_s this reference reaches and dT_s a rotation by 0.8^s 0.05 rad and a
    shift by 0.8^s 0.1 m in random directions: the step's solution is dT_s."""
    rng = np.random.default_rng(61)
    q = rng.uniform(-5, 5, (RING_GROUP, 3)).astype(f32)
    prm = dict(max_iter=1000, smooth=1, min_rot=0.0, min_trans=0.0)
    st = State()
    reads = []
    for s in range(RING_STEPS):
        ax, t = rng.normal(size=3), rng.normal(size=3)
        t *= 0.1 * RING_SHRINK ** s / np.linalg.norm(t)
        Rm = rot(ax, 0.05 * RING_SHRINK ** s)
        tgt = (q.astype(f64) - t) @ Rm                       # dT_s^-1 q
        Mt = st.T.astype(f64).reshape(4, 4).T
        Mi = np.linalg.inv(Mt)
        r = (tgt @ Mi[:3, :3].T + Mi[:3, 3]).astype(f32)
        reads.append(r)
        rows = np.zeros((1, COLS))
        rows[0, :NF] = products(apply_points(st.T, r), q).sum(axis=0)
        rows[0, 27] = RING_GROUP
        update(st, total_from_rows(rows), RING_STEPS * RING_GROUP, prm)
    n = RING_STEPS * RING_GROUP
    match = (np.arange(n) % RING_GROUP).astype(np.int32)
    d2 = [np.where(np.arange(n) // RING_GROUP == s, f32(0.25), f32(1.0)).astype(f32) for s in range(RING_STEPS)]
    touched = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(RING_STEPS)]
    return dict(q=q, nrm=np.zeros((RING_GROUP, 3), f32), r=np.concatenate(reads), match=match, d2=d2, touched=touched,
                limit=f32(0.5))


def case_ring(smooth):
    """40 steps, max_iter 64; min_rot / min_trans halfway (geometrically) between the smoothed
    differences of steps 34 and 35, so the pair converges at step 35, with hist_count past 32."""
    free = sr._batch([_ring_base()], n_steps=RING_STEPS, max_iter=64, smooth=smooth, min_rot=0.0, min_trans=0.0)
    cv = compare(free, simulate(free))["cv"]
    a, b = cv[RING_CONVERGES - 2][0], cv[RING_CONVERGES - 1][0]
    assert a[0] > b[0] and a[1] > b[1]
    return sr._batch([_ring_base()], n_steps=RING_STEPS, max_iter=64, smooth=smooth,
                     min_rot=float(f32(math.sqrt(a[0] * b[0]))), min_trans=float(f32(math.sqrt(a[1] * b[1]))))


def case_counter():
    """The same 40 steps with max_iter 36 and thresholds of 0: the counter stops the pair."""
    return sr._batch([_ring_base()], n_steps=RING_STEPS, max_iter=36, smooth=4, min_rot=0.0, min_trans=0.0)


CASES = {name: functools.partial(sr.get_case, name) for name in SHARED}
CASES.update(exact=case_exact, reflection=case_reflection, ranks=case_p2p_ranks, threshold=case_p2p_threshold,
             counter=case_counter)
CASES.update({f"ring{k}": functools.partial(case_ring, k) for k in RING_SMOOTH})


@functools.lru_cache(maxsize=None)
def get_case(name):
    return CASES[name]()


def entry_args(**over):
    """ctypes arguments of aicp_hip_test_step_p2p: step_reference.entry_args without ref_nrm."""
    args, keep = sr.entry_args(**over)
    i = list(keep).index("ref_nrm")
    return args[:i] + args[i + 1:], keep


# ------------------------------------------------------------------ whole runs --------------
def chain_text(minimizer="PointToPointErrorMinimizer", ratio=0.75, max_iter=100, min_rot=1e-4, min_trans=1e-4,
               smooth=4, ref_normals=True, extra_filter=None):
    """A libpointmatcher chain with the parameter values of the 2-D testing chain: SurfaceNormal knn
    10 on both clouds, KDTreeMatcher knn 1 epsilon 0, TrimmedDist 0.75, the minimizer, Counter 100 and
    Differential 1e-4 / 1e-4 / 4."""
    sn = "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
    read = "readingDataPointsFilters:\n" + (extra_filter or "") + sn
    ref = ("referenceDataPointsFilters:\n" + sn) if ref_normals else ""
    return (f"{read}\n{ref}\nmatcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n\n"
            f"outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: {ratio}\n\n"
            f"errorMinimizer:\n  {minimizer}\n\n"
            f"transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: {max_iter}\n"
            f"  - DifferentialTransformationChecker:\n      minDiffRotErr: {min_rot}\n"
            f"      minDiffTransErr: {min_trans}\n      smoothLength: {smooth}\n\n"
            "inspector:\n  NullInspector\n\nlogger:\n  NullLogger\n")


def _fixed40_mean(x):
    """icp_math.hpp fixed40 / mean_from_fixed40: the order-independent reference centroid."""
    v = np.rint(x.astype(f64) * 1099511627776.0)
    S = sum(int(t) for t in v)
    m = float(abs(S)) * (1.0 / 1099511627776.0) / float(len(x))
    return f32(-m if S < 0 else m)


def icp_reference(ref, read, ratio=0.75, max_iter=100, min_rot=1e-4, min_trans=1e-4, smooth=4, eps=0.0, bucket=8,
                  margin=(2e-6, 2e-5)):
    """A whole point-to-point run in numpy (the oracle's ICP::compute restatement with this module's
    update): centred reference, pyoracle.Tree.knn (libnabo order, the chain's epsilon),
    pyoracle.dists_quantile, fsum sums, the restated update. Raises MarginError when a smoothed
    cv0 / cv1 comes within `margin` (rad, m) of its threshold at any iteration: the device's
    transforms may differ from this loop's by the parity bar (1e-6 rad, 1e-5 m) each, two consecutive
    ones by twice that, so iteration counts are comparable only outside it.
    Returns dict(T (4x4 row-major float32), iterations, converged, status, kept, cv)."""
    import pyoracle as po

    ref = np.ascontiguousarray(ref, f32)[:, :3]
    read = np.ascontiguousarray(read, f32)[:, :3]
    mean = np.array([_fixed40_mean(ref[:, d]) for d in range(3)], f32)
    refc = (ref - mean).astype(f32)
    tree = po.Tree(refc, bucket)
    Tmean = sr.ident16()
    Tmean[12:15] = mean
    TrmDin = sr.ident16()
    TrmDin[12:15] = -mean
    rd = apply_points(TrmDin, read)
    prm = dict(max_iter=max_iter, smooth=smooth, min_rot=min_rot, min_trans=min_trans)
    st = State()
    out = dict(kept=[], cv=[])
    n = len(rd)
    while st.active:
        step = apply_points(st.T, rd)
        ids, d2, _, _ = tree.knn(step, 1, eps)
        ids, d2 = ids[:, 0], d2[:, 0]
        limit, qerr = po.dists_quantile(d2, ratio)
        if qerr:
            st.status, st.active = 1, 0
            break
        with np.errstate(invalid="ignore"):
            idx = np.nonzero(d2 <= f32(limit))[0]
        prod = products(step[idx], refc[ids[idx]])
        tot = np.zeros(COLS)
        tot[:NF] = [math.fsum(prod[:, c].tolist()) for c in range(NF)]
        tot[27] = len(idx)
        u = update(st, tot, n, prm)
        out["kept"].append(len(idx))
        out["cv"].append((u["cv0"], u["cv1"]))
        if u["cv0"] is not None:
            for cv, thr, mg, what in ((u["cv0"], float(f32(min_rot)), margin[0], "cv0"),
                                      (u["cv1"], float(f32(min_trans)), margin[1], "cv1")):
                if abs(cv - thr) < mg:
                    raise MarginError(f"iteration {st.iters}: {what} {cv!r} within {mg} of {thr!r}")
    T = mul4(mul4(Tmean, st.T), TrmDin)
    status = st.status
    if status == 0 and not rigid_ok(T):
        status = 5
    out.update(T=T.reshape(4, 4).T.copy(), iterations=st.iters, converged=st.converged, status=status)
    return out
