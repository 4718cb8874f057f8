"""Plain-numpy restatement of the tail of an ICP iteration, k_icp_reduce + k_icp_update_f: the
reference of test_step_kernels.py (Context.test_step / aicp_hip_test_step).

Terms. p = T r, F = (p x n, n) and dot = (p - q) . n in float32, one rounded operation at a time
in the order of apply4 and icp_reduce_body (the library is built with -ffp-contract=off, so these
are the device's floats). A product of two floats is exact in double.

Sums. Each of the 27 floating columns of a slab row, and of the sum over a pair's rows, is compared
with math.fsum of its exact products. A double sum of n exact addends t_i in any order is within
n 2^-53 sum|t_i| of the true sum to first order; the bound used is (n + 2) 2^-53 sum|t_i| (the two
extra units cover fsum's own rounding and the subtraction), n = the kept count of the row / pair.
Columns 27..29 (kept, touched points, touched nodes) are integers and must be equal. Rows of an
inactive pair must hold the sentinel the entry filled the slab with.

Update, bit for bit. From the device's own slab rows: tot in icp_update_body's order (group g sums
rows g, g + 8, ... in order, then the 8 groups are added in order), oracle.solve6, and
delta_transform, mul4, rigid_ok, quat_from_T, quat_angdist and update_serial's checkers restated in
numpy scalars of the same widths. T_iter, kept, iters, status, active, converged, hist_count,
inlier_ratio and the touch counters must equal the device's exactly, dt exactly (sqrt is correctly
rounded on both sides), dq within 4 ulp of double.

Not bit-exact: sin, cos and atan2 in double may differ between the device's math library and
Python's by a few ulp. The reference asserts that this cannot change an answer and raises
MarginError otherwise: sin(angle) and cos(angle) lie at least 2^-45 relative away from a float
rounding boundary, and the smoothed cv0 / cv1 at least 1e-9 relative away from min_rot / min_trans.

simulate() makes "device outputs" from the reference itself (optionally with one of MUTATIONS built
in), compare() checks device outputs; CASES is the table of inputs the GPU tests run, iterated by
the CPU tests for the margins.
"""
import functools
import math

import numpy as np

f32 = np.float32
f64 = np.float64
RB = 1024          # kReduceBlock: readings per slab row
COLS = 30          # kRedCols
RING = 32          # kHistRing
GROUPS = 8         # 256 / kRedCols
U = 2.0 ** -53
SENTINEL_BITS = 0x7FF8DEAD7FF8DEAD
QH, TH, DQ, DT, RING_WORDS = 0, 4 * RING, 7 * RING, 8 * RING, 9 * RING   # PairState's ring arrays, in doubles
MUTATIONS = ("lt", "drop_tail", "ref_off", "swapF", "rows128", "ring", "fullrank")


class Mismatch(AssertionError):
    """Device outputs differ from the reference."""


class MarginError(ValueError):
    """An input on which a few ulp of sin / cos / atan2 could change an answer."""


def _need(ok, msg):
    if not ok:
        raise Mismatch(msg)


# ------------------------------------------------------------------ float32 pieces ----------
def ident16():
    return np.eye(4, dtype=f32).reshape(16)


def apply_points(T, r):
    """apply4 on every row of r (k, 3): ((T0 x + T1 y) + T2 z) + T3 per row, in float32."""
    T = np.asarray(T, f32)
    r = np.asarray(r, f32)
    out = np.empty((r.shape[0], 3), f32)
    with np.errstate(all="ignore"):
        for i in range(3):
            s = T[i] * r[:, 0]
            s = s + T[4 + i] * r[:, 1]
            s = s + T[8 + i] * r[:, 2]
            out[:, i] = s + T[12 + i]
    return out


def terms(T, r, q, n, swapF=False):
    """F (k, 6) and dot (k,) in float32 for readings r, matched points q and normals n (k, 3)."""
    with np.errstate(all="ignore"):
        p = apply_points(T, r).T
        F = np.empty((r.shape[0], 6), f32)
        F[:, 0] = p[1] * n[:, 2] - p[2] * n[:, 1]
        F[:, 1] = p[2] * n[:, 0] - p[0] * n[:, 2]
        F[:, 2] = p[0] * n[:, 1] - p[1] * n[:, 0]
        F[:, 3:] = n
        if swapF:
            F[:, [1, 2]] = F[:, [2, 1]]
        dot = (p[0] - q[:, 0]) * n[:, 0]
        dot = dot + (p[1] - q[:, 1]) * n[:, 1]
        dot = dot + (p[2] - q[:, 2]) * n[:, 2]
    assert F.dtype == f32 and dot.dtype == f32
    return F, dot


def products(F, dot):
    """(k, 27) exact doubles: the 21 products F[a] F[b], a <= b, then the 6 products F[a] dot."""
    with np.errstate(all="ignore"):
        F = F.astype(f64)
        d = dot.astype(f64)
        cols = [F[:, a] * F[:, b] for a in range(6) for b in range(a, 6)] + [F[:, a] * d for a in range(6)]
    return np.stack(cols, axis=1) if len(d) else np.zeros((0, 27))


def mul4(A, B):
    C = np.empty(16, f32)
    for c in range(4):
        for r in range(4):
            s = A[r] * B[c * 4]
            s = s + A[4 + r] * B[c * 4 + 1]
            s = s + A[8 + r] * B[c * 4 + 2]
            s = s + A[12 + r] * B[c * 4 + 3]
            C[c * 4 + r] = s
    return C


def rigid_ok(T):
    m = lambda r, c: T[c * 4 + r]
    d0 = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1))
    d1 = m(1, 0) * (m(0, 1) * m(2, 2) - m(0, 2) * m(2, 1))
    d2 = m(2, 0) * (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1))
    det = (d0 - d1) + d2
    return not (abs(f32(1) - det) > f32(0.001))


def _rounding_margin(v, what):
    """v (double) rounds to the same float whatever few ulp a math library adds."""
    v = float(v)
    if not math.isfinite(v) or v == 0.0:
        return
    f = f32(v)
    if float(f) == v:
        return  # half a float ulp from either boundary
    other = np.nextafter(f, f32(np.inf) if float(f) < v else f32(-np.inf))
    mid = (float(f) + float(other)) / 2  # exact in double
    if abs(v - mid) < 2.0 ** -45 * abs(v):
        raise MarginError(f"{what} = {v!r} is within 2^-45 of a float rounding boundary")


def delta_transform(x):
    """x: 6 float32 (rotation vector, translation) -> 16 float32, Eigen::AngleAxis semantics."""
    sq = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    angle = np.sqrt(sq)
    axis = [x[0], x[1], x[2]]
    if sq > f32(0):
        axis = [x[i] / angle for i in range(3)]
    sd, cd = np.sin(f64(angle)), np.cos(f64(angle))
    _rounding_margin(sd, "sin(angle)")
    _rounding_margin(cd, "cos(angle)")
    sa, c = f32(sd), f32(cd)
    sin_axis = [sa * a for a in axis]
    cos1_axis = [(f32(1) - c) * a for a in axis]
    R = np.zeros((3, 3), f32)
    tmp = cos1_axis[0] * axis[1]
    R[0, 1] = tmp - sin_axis[2]
    R[1, 0] = tmp + sin_axis[2]
    tmp = cos1_axis[0] * axis[2]
    R[0, 2] = tmp + sin_axis[1]
    R[2, 0] = tmp - sin_axis[1]
    tmp = cos1_axis[1] * axis[2]
    R[1, 2] = tmp - sin_axis[0]
    R[2, 1] = tmp + sin_axis[0]
    for i in range(3):
        R[i, i] = cos1_axis[i] * axis[i] + c
    T = np.zeros(16, f32)
    for r in range(3):
        for cc in range(3):
            T[cc * 4 + r] = R[r, cc]
        T[12 + r] = x[3 + r]
    T[15] = 1
    if np.isnan(R).any() or any(np.isnan(x[3 + r]) for r in range(3)):
        for r in range(3):
            for cc in range(3):
                T[cc * 4 + r] = 1 if r == cc else 0
    return T


# ------------------------------------------------------------------ double pieces -----------
def _sqrt(x):
    return f64(math.sqrt(x)) if x >= 0 else f64(np.nan)


def quat_from_T(T):
    m = [[f64(T[c * 4 + r]) for c in range(3)] for r in range(3)]
    q = [f64(0)] * 4
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0:
        t = _sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2][1] - m[1][2]) * t
        q[2] = (m[0][2] - m[2][0]) * t
        q[3] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        v = [None] * 3
        v[i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k][j] - m[j][k]) * t
        v[j] = (m[j][i] + m[i][j]) * t
        v[k] = (m[k][i] + m[i][k]) * t
        q[1:] = v
    return [f64(v) for v in q]


def quat_angdist(a, b):
    bw, bx, by, bz = b[0], -b[1], -b[2], -b[3]
    w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz
    x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by
    y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz
    z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx
    return f64(2.0 * math.atan2(float(_sqrt(x * x + y * y + z * z)), float(abs(w))))


def total_from_rows(rows, mut=None):
    """icp_update_body's order: group g sums rows g, g + 8, ... in order, then the groups in order."""
    with np.errstate(all="ignore"):
        part = []
        for g in range(GROUPS):
            v = np.zeros(COLS)
            for r in range(g, rows.shape[0], GROUPS):
                if mut == "rows128" and r >= 16 * GROUPS:
                    continue
                v = v + rows[r]
            part.append(v)
        tot = part[0]
        for g in range(1, GROUPS):
            tot = tot + part[g]
    return tot


def normal_system(tot):
    A = np.zeros((6, 6))
    c = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = tot[c]
            c += 1
    return A, -tot[21:27]


def _llt6(A, b):
    """llt_solve<6>'s arithmetic whatever the pivots (the `fullrank` mutation)."""
    with np.errstate(all="ignore"):
        L = np.zeros((6, 6))
        for j in range(6):
            L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
        y = np.zeros(6)
        x = np.zeros(6)
        for i in range(6):
            y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
        for i in range(5, -1, -1):
            x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def solve6(A, b, mut=None):
    import pyoracle

    x, path = pyoracle.solve6(A, b)
    if mut == "fullrank" and path != 0:
        return _llt6(A, b), 0
    return x, path


class State:
    """PairState as k_init_state leaves it (the ring's entry 0 is the identity's), then init_T."""

    def __init__(self, T0=None, active=True):
        self.T = ident16()
        self.ring = np.zeros(RING_WORDS + 8 * RING)  # (room for the `ring` mutation's indices)
        self.ring[QH:QH + 4] = quat_from_T(self.T)
        if T0 is not None:
            self.T = np.array(T0, f32).reshape(16)
        self.limit = f32(0)
        self.active = int(bool(active))
        self.status = self.iters = self.converged = self.kept = 0
        self.hist_count = 1
        self.inlier_ratio = f32(0)
        self.touched_pts = self.touched_nodes = 0

    def last_dqdt(self):
        h = (self.hist_count - 1) % RING
        return self.ring[DQ + h], self.ring[DT + h]


def update(st, tot, n_read, prm, mut=None):
    """update_serial on the sums tot; returns dict(path, cv0, cv1) (None where not reached)."""
    info = dict(path=None, cv0=None, cv1=None)
    ix = (lambda h: h) if mut == "ring" else (lambda h: h % RING)
    with np.errstate(all="ignore"):
        st.touched_pts += int(tot[28])
        st.touched_nodes += int(tot[29])
        kept = int(tot[27])
        st.kept = kept
        if kept == 0:
            st.status, st.active = 1, 0
            return info
        A, b = normal_system(tot)
        xd, info["path"] = solve6(A, b, mut)
        x = [f32(v) for v in xd]
        st.T = mul4(delta_transform(x), st.T)
        st.inlier_ratio = f32(f64(f32(kept)) / f64(n_read))
        if not rigid_ok(st.T):
            st.iters += 1
            st.status, st.active = 5, 0
            return info
        iterate = True
        st.iters += 1
        if st.iters >= prm["max_iter"]:
            iterate = False
        R = st.ring
        h = ix(st.hist_count)
        R[QH + 4 * h:QH + 4 * h + 4] = quat_from_T(st.T)
        R[TH + 3 * h:TH + 3 * h + 3] = [f64(st.T[12 + i]) for i in range(3)]
        if st.hist_count >= 1:
            bp = ix(st.hist_count - 1)
            R[DQ + h] = abs(quat_angdist(R[QH + 4 * h:QH + 4 * h + 4], R[QH + 4 * bp:QH + 4 * bp + 4]))
            d = R[TH + 3 * h:TH + 3 * h + 3] - R[TH + 3 * bp:TH + 3 * bp + 3]
            R[DT + h] = _sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        st.hist_count += 1
        sz = st.hist_count
        if sz > prm["smooth"]:
            cv0 = cv1 = f64(0)
            for i in range(sz - 1, sz - prm["smooth"] - 1, -1):
                cv0 = cv0 + R[DQ + ix(i)]
                cv1 = cv1 + R[DT + ix(i)]
            cv0 = cv0 / prm["smooth"]
            cv1 = cv1 / prm["smooth"]
            info["cv0"], info["cv1"] = float(cv0), float(cv1)
            if cv0 != cv0 or cv1 != cv1:
                st.status, st.active = 1, 0
                return info
            mr, mt = float(f32(prm["min_rot"])), float(f32(prm["min_trans"]))
            for cv, thr, what in ((cv0, mr, "cv0 against min_rot"), (cv1, mt, "cv1 against min_trans")):
                if thr > 0 and abs(float(cv) - thr) < 1e-9 * thr:
                    raise MarginError(f"{what}: {float(cv)!r} within 1e-9 of {thr!r}")
            if cv0 < mr and cv1 < mt:
                if iterate:
                    st.converged = 1
                iterate = False
        st.active = 1 if iterate else 0
    return info


# ------------------------------------------------------------------ a case's geometry -------
def layout(case):
    n_read = np.asarray(case["n_read"], np.int64)
    offs = np.concatenate([[0], np.cumsum(n_read)])
    nrow = (n_read + RB - 1) // RB
    roff = np.concatenate([[0], np.cumsum(nrow)])
    return n_read, offs, nrow, roff


def params(case):
    return dict(max_iter=int(case.get("max_iter", 20)), smooth=int(case.get("smooth", 4)),
                min_rot=case.get("min_rot", 1e-3), min_trans=case.get("min_trans", 1e-2))


def initial_states(case):
    P = len(case["n_read"])
    T0 = case.get("init_T")
    act = case.get("active")
    return [State(None if T0 is None else np.asarray(T0, f32).reshape(P, 16)[p], True if act is None else act[p])
            for p in range(P)]


def pair_terms(case, s, p, T, limit, mut=None):
    """The kept readings of pair p in step s: their indices, exact products (k, 27), and the touch
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
    ref_nrm = np.asarray(case["ref_nrm"], f32).reshape(-1, 3)
    g = int(case["ref_off"][p]) + (1 if mut == "ref_off" and p == 1 else 0) + match[idx].astype(np.int64)
    g = np.minimum(g, ref_pts.shape[0] - 1)
    r = np.asarray(case["read_c"], f32).reshape(-1, 3)[o + idx]
    F, dot = terms(np.asarray(T, f32), r, ref_pts[g], ref_nrm[g], swapF=mut == "swapF")
    return idx, products(F, dot), (tc & 0xFFFF) * read, (tc >> 16) * read


def own_rows(idx, prod, tp, tn, nrow):
    """Slab rows from the reference's own (numpy) sums."""
    rows = np.zeros((nrow, COLS))
    with np.errstate(all="ignore"):
        for r in range(nrow):
            sel = (idx // RB) == r
            rows[r, :27] = prod[sel].sum(axis=0)
            rows[r, 27] = int(sel.sum())
            rows[r, 28] = int(tp[r * RB:(r + 1) * RB].sum())
            rows[r, 29] = int(tn[r * RB:(r + 1) * RB].sum())
    return rows


def _check_sum(dev, col, k, what):
    if np.isnan(col).any():
        _need(np.isnan(dev), f"{what}: {dev!r} where a term is NaN")
        return
    exact = math.fsum(col.tolist())
    bound = (k + 2) * U * math.fsum(np.abs(col).tolist())
    _need(math.isfinite(dev) and abs(dev - exact) <= bound, f"{what}: {dev!r} against {exact!r}, bound {bound!r}")


def check_slab(dev_rows, idx, prod, tp, tn, what, mut=None):
    """A pair's device rows, and their total in the update's order, against the exact sums."""
    nrow = dev_rows.shape[0]
    rid = idx // RB
    for r in range(nrow):
        sel = rid == r
        k = int(sel.sum())
        want = (k, int(tp[r * RB:(r + 1) * RB].sum()), int(tn[r * RB:(r + 1) * RB].sum()))
        got = tuple(dev_rows[r, 27:])
        _need(got == tuple(float(v) for v in want), f"{what} row {r}: kept / touched {got} against {want}")
        for c in range(27):
            _check_sum(float(dev_rows[r, c]), prod[sel, c], k, f"{what} row {r} column {c}")
    tot = total_from_rows(dev_rows, mut)
    want = (len(idx), int(tp.sum()), int(tn.sum()))
    _need(tuple(tot[27:]) == tuple(float(v) for v in want), f"{what} totals: kept / touched {tuple(tot[27:])} against {want}")
    for c in range(27):
        _check_sum(float(tot[c]), prod[:, c], len(idx), f"{what} total column {c}")
    return tot


INT_KEYS = ("kept", "iters", "status", "active", "converged", "hist_count")


def _record(out, s, p, st):
    out["T"][s, p] = st.T
    for k in INT_KEYS:
        out[k][s, p] = getattr(st, k)
    out["inlier_ratio"][s, p] = st.inlier_ratio
    out["touched_pts"][s, p] = st.touched_pts
    out["touched_nodes"][s, p] = st.touched_nodes
    out["dq"][s, p], out["dt"][s, p] = st.last_dqdt()


def _empty(case):
    _, _, nrow, roff = layout(case)
    S, P = np.asarray(case["limit"]).shape
    out = dict(slab=np.zeros((S, int(roff[-1]), COLS)), T=np.zeros((S, P, 16), f32),
               inlier_ratio=np.zeros((S, P), f32), touched_pts=np.zeros((S, P), np.uint64),
               touched_nodes=np.zeros((S, P), np.uint64), dq=np.zeros((S, P)), dt=np.zeros((S, P)), dirty=0)
    for k in INT_KEYS:
        out[k] = np.zeros((S, P), np.int32)
    return out


def simulate(case, mut=None):
    """What Context.test_step would return if the device were this reference (with `mut` built in)."""
    n_read, _, nrow, roff = layout(case)
    prm = params(case)
    out = _empty(case)
    out["slab"].view(np.uint64)[:] = SENTINEL_BITS
    states = initial_states(case)
    S, P = out["kept"].shape
    for s in range(S):
        for p, st in enumerate(states):
            if st.active:
                st.limit = f32(np.asarray(case["limit"], f32)[s, p])
                idx, prod, tp, tn = pair_terms(case, s, p, st.T, st.limit, mut)
                rows = own_rows(idx, prod, tp, tn, int(nrow[p]))
                out["slab"][s, roff[p]:roff[p + 1]] = rows
                update(st, total_from_rows(rows, mut), int(n_read[p]), prm, mut)
            _record(out, s, p, st)
    return out


def _same_floats(a, b):
    a, b = np.asarray(a), np.asarray(b)
    bits = np.uint32 if a.dtype == f32 else np.uint64
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def ulp_diff(a, b):
    a, b = f64(a), f64(b)
    if np.isnan(a) and np.isnan(b):
        return 0
    if np.isnan(a) or np.isnan(b):
        return 2 ** 63
    return abs(int(a.view(np.int64)) - int(b.view(np.int64)))


def compare(case, got):
    """Device outputs against the reference; raises Mismatch. Returns dict(max_dq_ulp, paths, cv):
    paths[s][p] the solve6 path the oracle took on the device's totals (None: no solve), cv[s][p]
    the smoothed (cv0, cv1)."""
    n_read, _, nrow, roff = layout(case)
    prm = params(case)
    want = _empty(case)
    states = initial_states(case)
    S, P = want["kept"].shape
    _need(got["slab"].shape == want["slab"].shape, "slab shape")
    info = dict(max_dq_ulp=0, paths=[], cv=[])
    for s in range(S):
        info["paths"].append([None] * P)
        info["cv"].append([None] * P)
        for p, st in enumerate(states):
            dev = got["slab"][s, roff[p]:roff[p + 1]]
            what = f"step {s} pair {p}"
            if st.active:
                st.limit = f32(np.asarray(case["limit"], f32)[s, p])
                idx, prod, tp, tn = pair_terms(case, s, p, st.T, st.limit)
                tot = check_slab(dev, idx, prod, tp, tn, what)
                u = update(st, tot, int(n_read[p]), prm)
                info["paths"][s][p] = u["path"]
                info["cv"][s][p] = (u["cv0"], u["cv1"])
            else:
                _need(bool(np.all(np.ascontiguousarray(dev).view(np.uint64) == SENTINEL_BITS)),
                      f"{what}: an inactive pair's rows were written")
            _record(want, s, p, st)
            _need(_same_floats(got["T"][s, p], want["T"][s, p]), f"{what}: T_iter {got['T'][s, p]} against {want['T'][s, p]}")
            for k in INT_KEYS + ("touched_pts", "touched_nodes"):
                _need(int(got[k][s, p]) == int(want[k][s, p]), f"{what}: {k} {got[k][s, p]} against {want[k][s, p]}")
            _need(_same_floats(got["inlier_ratio"][s, p], want["inlier_ratio"][s, p]), f"{what}: inlier_ratio")
            _need(_same_floats(got["dt"][s, p], want["dt"][s, p]), f"{what}: dt {got['dt'][s, p]!r} against {want['dt'][s, p]!r}")
            d = ulp_diff(got["dq"][s, p], want["dq"][s, p])
            info["max_dq_ulp"] = max(info["max_dq_ulp"], d)
            _need(d <= 4, f"{what}: dq {got['dq'][s, p]!r} against {want['dq'][s, p]!r}: {d} ulp")
    _need(got["dirty"] == 0, f"{got['dirty']} arrival counters left non-zero")
    return info


# ------------------------------------------------------------------ the cases ---------------
def _scene(rng, n_ref, kind="general", s=0.0):
    """Reference points in a 10 m box and unit normals (float32): general; `noX` normals without an
    x component (one degenerate direction); `z` all (0, 0, 1); `zs`: z + s e, e a unit vector in xy."""
    q = rng.uniform(-5, 5, (n_ref, 3))
    if kind == "general":
        n = rng.normal(size=(n_ref, 3))
    elif kind == "noX":
        a = rng.uniform(0, 2 * np.pi, n_ref)
        n = np.stack([np.zeros(n_ref), np.cos(a), np.sin(a)], axis=1)
    else:
        a = rng.uniform(0, 2 * np.pi, n_ref)
        n = np.stack([s * np.cos(a), s * np.sin(a), np.ones(n_ref)], axis=1)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return q.astype(f32), n.astype(f32)


def _readings(rng, n, q, noise=0.02):
    """n readings near matched reference points; the matches include both ends of the reference."""
    match = rng.integers(0, len(q), n).astype(np.int32)
    match[0] = 0
    match[-1] = len(q) - 1
    r = (q[match] + noise * rng.normal(size=(n, 3))).astype(f32)
    d2 = (rng.exponential(size=n) + 1e-3).astype(f32)
    touched = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return r, match, d2, touched


def _limit(d2, ratio):
    """A limit that keeps none (0), about half (0.5) or all (1) of the finite distances."""
    f = np.sort(d2[np.isfinite(d2)])
    return f32(-1.0) if ratio == 0 else f[-1] if ratio == 1 else f[len(f) // 2]


def _batch(pairs, n_steps=1, **prm):
    """pairs: dicts(q, nrm, r, match, d2, touched, limit[, own_ref]) -> a case. match / d2 /
    touched / limit: one array or a list of n_steps. A pair without q shares the previous pair's
    reference range."""
    n_read, n_ref, ref_off, qs, ns = [], [], [], [], []
    off = 0
    for pr in pairs:
        if pr.get("q") is not None:
            ref_off.append(off)
            qs.append(pr["q"])
            ns.append(pr["nrm"])
            off += len(pr["q"])
        else:
            ref_off.append(ref_off[-1])
        n_ref.append(len(qs[-1]))
        n_read.append(len(pr["r"]))
    per = lambda pr, k, s: pr[k][s] if isinstance(pr[k], list) else pr[k]
    case = dict(n_read=n_read, n_ref=n_ref, ref_off=ref_off, read_c=np.concatenate([pr["r"] for pr in pairs]),
                ref_pts=np.concatenate(qs), ref_nrm=np.concatenate(ns),
                limit=np.array([[per(pr, "limit", s) for pr in pairs] for s in range(n_steps)], f32),
                match=np.stack([np.concatenate([per(pr, "match", s) for pr in pairs]) for s in range(n_steps)]),
                d2=np.stack([np.concatenate([per(pr, "d2", s) for pr in pairs]) for s in range(n_steps)]),
                touched=np.stack([np.concatenate([per(pr, "touched", s) for pr in pairs]) for s in range(n_steps)]))
    case.update(prm)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _simple_pair(rng, n, q, nrm, ratio=1.0, own=True):
    r, match, d2, touched = _readings(rng, n, q)
    return dict(q=q if own else None, nrm=nrm, r=r, match=match, d2=d2, touched=touched, limit=_limit(d2, ratio))


TAILS = (1, 255, 256, 257, 1023, 1024, 1025, 4097)


def case_tail(n):
    """Three pairs of n readings on one shared 64-point reference: none, about half and all kept."""
    rng = np.random.default_rng(100 + n)
    q, nrm = _scene(rng, 64)
    return _batch([_simple_pair(rng, n, q, nrm, ratio, own=i == 0) for i, ratio in enumerate((0, 0.5, 1))])


def case_ties():
    """600 readings: 100 at d2 == limit exactly, 50 at nextafter(limit, inf), 20 at +inf and 20 NaN
    (both unmatched, -1), the rest on both sides."""
    rng = np.random.default_rng(7)
    q, nrm = _scene(rng, 64)
    pr = _simple_pair(rng, 600, q, nrm)
    lim = f32(0.7)
    d2 = pr["d2"].copy()
    match = pr["match"].copy()
    slot = rng.permutation(600)
    d2[slot[:100]] = lim
    d2[slot[100:150]] = np.nextafter(lim, f32(np.inf))
    d2[slot[150:170]] = np.inf
    d2[slot[170:190]] = np.nan
    match[slot[150:190]] = -1
    pr.update(d2=d2, match=match, limit=lim)
    return _batch([pr])


RAGGED = (1, 1025, 300, 5000, 2048)


def case_ragged():
    """Five pairs of RAGGED readings on references of 64, 100, 37, 200 and 90 points, the third
    inactive from the start, and a sixth with the second's inputs on a copy of its reference;
    two steps."""
    rng = np.random.default_rng(11)
    pairs = []
    for n, m in zip(RAGGED, (64, 100, 37, 200, 90)):
        q, nrm = _scene(rng, m)
        a, b = _simple_pair(rng, n, q, nrm, 0.5), _simple_pair(rng, n, q, nrm, 1.0)
        for k in ("match", "d2", "touched", "limit"):
            a[k] = [a[k], b[k]]
        pairs.append(a)
    pairs.append(dict(pairs[1]))
    return _batch(pairs, n_steps=2, active=[1, 1, 0, 1, 1, 1])


def case_rows129():
    """One pair of 131073 + 700 readings: 129 slab rows, the update's second pass over r0."""
    rng = np.random.default_rng(13)
    q, nrm = _scene(rng, 64)
    return _batch([_simple_pair(rng, 131073 + 700, q, nrm, 0.5)])


def case_touch():
    """70001 readings whose touch words have both halves up to 0xFFFF (half of them 0xFFFFFFFF),
    three steps: the totals pass 2^32."""
    rng = np.random.default_rng(17)
    q, nrm = _scene(rng, 64)
    pr = _simple_pair(rng, 70001, q, nrm, 0.5)
    t = []
    for s in range(3):
        w = rng.integers(0, 1 << 32, 70001, dtype=np.uint64).astype(np.uint32)
        w[rng.random(70001) < 0.5] = 0xFFFFFFFF
        t.append(w)
    pr["touched"] = t
    return _batch([pr], n_steps=3)


RANKS = (6, 5, 3, 1)


def case_ranks():
    """Four pairs whose systems have rank 6, 5, 3 and 1: a general scene, normals without an x
    component, all normals z, a single kept reading; two steps."""
    rng = np.random.default_rng(19)
    pairs = []
    for kind in ("general", "noX", "z", "general"):
        q, nrm = _scene(rng, 64, kind)
        pairs.append(_simple_pair(rng, 700, q, nrm, 0.5))
    pairs[3]["limit"] = pairs[3]["d2"].min()
    return _batch(pairs, n_steps=2)


THRESHOLD_S = (1e-6, 1e-5, 1e-4, 1e-3) + tuple(float(10.0 ** (-2.75 + 0.125 * k)) for k in range(7)) + (3e-2, 1e-1)


def case_threshold():
    """Normals z + s e, one pair per s in THRESHOLD_S: from 1e-6, where the three weak directions
    fall below the pivoted-QR rank threshold (6 FLT_EPSILON of the largest pivot) and the rank-3
    minimal-norm solution leaves no residual (path 1), through the threshold in steps of 10^0.125
    (rank-deficient with a residual: the pseudo-inverse, path 2), to 0.1 (full rank, LLT, path 0);
    two steps."""
    rng = np.random.default_rng(23)
    pairs = []
    for s in THRESHOLD_S:
        q, nrm = _scene(rng, 64, "zs", s)
        pairs.append(_simple_pair(rng, 500, q, nrm, 0.5))
    return _batch(pairs, n_steps=2)


def _rigid(yaw, t):
    c, s = math.cos(yaw), math.sin(yaw)
    M = np.array([[c, -s, 0, t[0]], [s, c, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1]])
    return M.T.reshape(16).astype(f32)  # column-major


def case_none_kept():
    """No reading within the limit: status 1 ("no point to minimize"), T_iter unchanged."""
    rng = np.random.default_rng(29)
    q, nrm = _scene(rng, 64)
    return _batch([_simple_pair(rng, 300, q, nrm, 0)], n_steps=2, init_T=_rigid(0.1, (0.3, -0.2, 0.1)))


def case_nonrigid():
    """T_iter starts as 1.002^(1/3) I (det R = 1.002): status 5 after one step."""
    rng = np.random.default_rng(31)
    q, nrm = _scene(rng, 64)
    T0 = ident16()
    T0[[0, 5, 10]] = f32(1.002 ** (1.0 / 3.0))
    return _batch([_simple_pair(rng, 300, q, nrm, 1.0)], n_steps=2, init_T=T0)


def case_nan_normal():
    """One kept reference point has a NaN normal; smooth 2, four steps."""
    rng = np.random.default_rng(37)
    q, nrm = _scene(rng, 64)
    nrm = nrm.copy()
    nrm[5] = np.nan
    pr = _simple_pair(rng, 300, q, nrm, 1.0)
    pr["match"][17] = 5
    return _batch([pr], n_steps=4, smooth=2)


RING_STEPS, RING_GROUP, RING_SHRINK = 40, 64, 0.8
RING_CONVERGES = 35  # the step (1-based) at which the thresholds of case_ring let the pair converge


@functools.lru_cache(maxsize=None)
def _ring_base():
    """2560 readings in 40 groups of 64; step s keeps group s alone (d2 0.25 against 1.0, limit 0.5),
    whose readings lie at T_s^-1 (q - w_s x q - t_s) for the T_s this reference reaches, so the
    step's solution is about (w_s, t_s) = 0.8^s (0.05 rad, 0.1 m) in random directions."""
    rng = np.random.default_rng(41)
    q, nrm = _scene(rng, RING_GROUP)
    prm = dict(max_iter=1000, smooth=1, min_rot=0.0, min_trans=0.0)
    st = State()
    reads = []
    for s in range(RING_STEPS):
        w, t = rng.normal(size=3), rng.normal(size=3)
        w *= 0.05 * RING_SHRINK ** s / np.linalg.norm(w)
        t *= 0.1 * RING_SHRINK ** s / np.linalg.norm(t)
        target = q.astype(f64) - np.cross(w, q.astype(f64)) - t
        M = st.T.astype(f64).reshape(4, 4).T
        Mi = np.linalg.inv(M)
        r = (target @ Mi[:3, :3].T + Mi[:3, 3]).astype(f32)
        reads.append(r)
        F, dot = terms(st.T, r, q, nrm)
        rows = np.zeros((1, COLS))
        rows[0, :27] = products(F, dot).sum(axis=0)
        rows[0, 27] = RING_GROUP
        update(st, total_from_rows(rows), RING_STEPS * RING_GROUP, prm)
    n = RING_STEPS * RING_GROUP
    match = (np.arange(n) % RING_GROUP).astype(np.int32)
    d2 = [np.where(np.arange(n) // RING_GROUP == s, f32(0.25), f32(1.0)).astype(f32) for s in range(RING_STEPS)]
    touched = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(RING_STEPS)]
    return dict(q=q, nrm=nrm, r=np.concatenate(reads), match=match, d2=d2, touched=touched, limit=f32(0.5))


RING_SMOOTH = (1, 4, 31)


def case_ring(smooth):
    """40 steps, max_iter 64; min_rot / min_trans halfway (geometrically) between the smoothed
    differences of steps 34 and 35, so the pair converges at step 35, with hist_count past 32."""
    free = _batch([_ring_base()], n_steps=RING_STEPS, max_iter=64, smooth=smooth, min_rot=0.0, min_trans=0.0)
    cv = compare(free, simulate(free))["cv"]
    a, b = cv[RING_CONVERGES - 2][0], cv[RING_CONVERGES - 1][0]
    assert a[0] > b[0] and a[1] > b[1]
    return _batch([_ring_base()], n_steps=RING_STEPS, max_iter=64, smooth=smooth,
                  min_rot=float(f32(math.sqrt(a[0] * b[0]))), min_trans=float(f32(math.sqrt(a[1] * b[1]))))


def case_counter():
    """The same 40 steps with max_iter 36 and thresholds of 0: the counter stops the pair."""
    return _batch([_ring_base()], n_steps=RING_STEPS, max_iter=36, smooth=4, min_rot=0.0, min_trans=0.0)


# name -> builder of every input the GPU tests run
CASES = {f"tail{n}": functools.partial(case_tail, n) for n in TAILS}
CASES.update(ties=case_ties, ragged=case_ragged, rows129=case_rows129, touch=case_touch, ranks=case_ranks,
             threshold=case_threshold, none_kept=case_none_kept, nonrigid=case_nonrigid, nan_normal=case_nan_normal,
             counter=case_counter)
CASES.update({f"ring{k}": functools.partial(case_ring, k) for k in RING_SMOOTH})


@functools.lru_cache(maxsize=None)
def get_case(name):
    return CASES[name]()


def entry_args(**over):
    """ctypes arguments of aicp_hip_test_step for a two-reading pair on a two-point reference;
    `over`: name -> replacement. Returns (args, keep-alive)."""
    import ctypes as C

    u32, i32, fl, u8, dbl, u64 = C.c_uint32, C.c_int32, C.c_float, C.c_uint8, C.c_double, C.c_uint64
    a = dict(ctx=C.c_void_p(1),   # never dereferenced: every check comes first
             n_pairs=1, n_read=(u32 * 1)(2), n_ref=(u32 * 1)(2), ref_off=(u32 * 1)(0), total_ref=2,
             read_c=(fl * 6)(), ref_pts=(fl * 6)(), ref_nrm=(fl * 6)(0, 0, 1, 0, 0, 1), init_T=None, active=None,
             max_iter=20, smooth=4, min_rot=1e-3, min_trans=1e-2, n_steps=1, limit=(fl * 1)(1.0),
             match=(i32 * 2)(0, 1), d2=(fl * 2)(0.5, 0.5), touched=(u32 * 2)(), out_slab=(dbl * 30)(),
             out_T=(fl * 16)(), out_state=(i32 * 6)(), out_inlier=(fl * 1)(), out_touched=(u64 * 2)(),
             out_dqdt=(dbl * 2)(), out_dirty=C.byref(u64()))
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values()), a
