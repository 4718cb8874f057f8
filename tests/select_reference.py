"""Plain-numpy restatement of the TrimmedDist limit (Matches::getDistsQuantile) and of what a
sequence of device selects leaves in a pair's state: the reference of test_select_kernels.py.

Per pair and step: the finite values f of the pair's distances, n = f.size,
k = n - 1 when ratio == 1, else min(int(float32(n) * float32(ratio)), n - 1) with the product taken
in float32 as getDistsQuantile takes it, limit = sort(f)[k]. The select is exact, so every
comparison against it is for equality (the limit as bits).

Input contract: what the NN kernel writes, non-negative floats (+0.0 and denormals included) or
+inf. NaN and -0.0 are outside it (the radix select orders values by their bit patterns).
"""
import numpy as np

FUSED = (2, 3, 4)  # variants of aicp_hip_test_select whose compaction runs on a guessed digit-1 bin
INF_BITS = 0x7F800000


def check_contract(d2):
    d2 = np.asarray(d2)
    assert d2.dtype == np.float32, d2.dtype
    bits = d2.view(np.uint32)
    assert np.all(bits <= INF_BITS), "distances must be non-negative floats or +inf (no NaN, no -0.0)"
    return d2


def kth_index(n, ratio):
    """Rank (0-based) of the limit among n finite values."""
    ratio = np.float32(ratio)
    if ratio == np.float32(1.0):
        return n - 1
    return min(int(np.float32(n) * ratio), n - 1)


def select_one(d2, ratio):
    """(limit, n_finite) of one pair's distances; limit None when no distance is finite."""
    d2 = check_contract(d2)
    f = d2[d2 != np.inf]
    n = int(f.size)
    if n == 0:
        return None, 0
    return np.sort(f)[kth_index(n, ratio)], n


def bin1(limit):
    """Digit 1 of the radix select: bits 31..21 of the value."""
    return int(np.float32(limit).view(np.uint32)) >> 21


def run_steps(d2_steps, counts, ratios, variants, active=None):
    """What Context.test_select returns (without dirty, which is 0): arrays (n_steps, n_pairs)."""
    counts = [int(c) for c in counts]
    P, S = len(counts), len(variants)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = dict(limit=np.zeros((S, P), np.float32), status=np.zeros((S, P), np.int32),
               n_finite=np.zeros((S, P), np.int32), b1=np.zeros((S, P), np.uint32),
               miss=np.zeros((S, P), np.uint32))
    on = [True] * P if active is None else [bool(a) for a in active]
    state = [dict(limit=np.float32(0), status=0, n_finite=0, b1=0, miss=0) for _ in range(P)]
    for s in range(S):
        d2 = check_contract(np.ascontiguousarray(d2_steps[s], np.float32).ravel())
        assert d2.size == offs[-1]
        for p in range(P):
            st = state[p]
            if on[p]:
                limit, n = select_one(d2[offs[p]:offs[p + 1]], ratios[p])
                if n == 0:  # ConvergenceError("no outlier to filter"): the pair stops, nothing else is written
                    st["status"] = 1
                    on[p] = False
                else:
                    b = bin1(limit)
                    if int(variants[s]) in FUSED and b != st["b1"]:
                        st["miss"] += 1
                    st.update(limit=limit, n_finite=n, b1=b)
            for key in out:
                out[key][s, p] = st[key]
    return out


def assert_equal(got, want, what=""):
    """Every output of a run against the reference: the limit as bits, the rest as integers."""
    for key in ("n_finite", "status", "b1", "miss"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")
    np.testing.assert_array_equal(got["limit"].view(np.uint32), want["limit"].view(np.uint32),
                                  err_msg=f"{what}: limit bits")
    assert got["dirty"] == 0, f"{what}: {got['dirty']} words of the select's work space left non-zero"
