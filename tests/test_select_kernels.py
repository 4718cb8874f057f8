"""The trimmed-limit select kernels, every variant, against the exact k-th smallest finite value.

Context.test_select (aicp_hip_test_select) runs a chosen select on given distances with the ICP
loop's set-up; select_reference.run_steps says what it must leave in each pair's state. Every
comparison is exact: the limit as bits, n_finite / status / b1 / miss as integers, and no word of
the self-resetting work space left non-zero. Variants: 0 separate launches (k_sel_hist, find1,
compact, final), 1 k_sel_hist_f + k_sel_compact_f, 2 k_sel_fused with the launcher's template,
3 k_sel_fused<kHistBins> (2048 candidates in LDS), 4 k_sel_fused<kFinalLds> (8192), 5 k_sel_pair
(12288, pairs of at most 65536 readings).

Float layout of the radix select: digit 1 = bits 31..21 (the bin b1), digit 2 = bits 20..10,
digit 3 = bits 9..0.
"""
import functools

import numpy as np
import pytest

import select_reference as sr

pytestmark = pytest.mark.gpu

from aicp_mapping_amd import synthetic as sy

ALL = (0, 1, 2, 3, 4, 5)
FUSED = (2, 3, 4)
BIN_ONE = 0x3F800000 >> 21  # the bin of [1.0, 1.25)
NEAR_ONE = np.nextafter(np.float32(1), np.float32(0))
RATIOS = (0.0, 0.25, 0.358818, 0.7, float(NEAR_ONE), 1.0)


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ value families ----------
def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


def spread(n, seed):
    """exponential^3 (values over ~100 digit-1 bins), every 13th value inf."""
    d2 = np.random.default_rng(seed).exponential(size=n).astype(np.float32) ** 3
    d2[12::13] = np.inf
    return d2


def one_bin(n, seed):
    """uniform in [1.0, 1.25): one digit-1 bin, the candidate count equals n."""
    return from_bits((BIN_ONE << 21) + np.random.default_rng(seed).integers(0, 1 << 21, n))


def one_value(n):
    return np.full(n, 0.37, np.float32)


def zeros(n, seed):
    """40 % exact 0.0, n // 200 denormals, the rest exponential^3 (all normal numbers)."""
    rng = np.random.default_rng(seed)
    nz, nd = n * 2 // 5, n // 200
    d2 = np.concatenate([np.zeros(nz, np.float32), from_bits(rng.integers(1, 1 << 23, nd)),
                         (rng.exponential(size=n - nz - nd).astype(np.float32) + np.float32(1e-3)) ** 3])
    return rng.permutation(d2)


def in_bins(parts, seed):
    """parts: (digit-1 bin, count) pairs; random low 21 bits in each bin, shuffled."""
    rng = np.random.default_rng(seed)
    b = np.concatenate([(int(bin_) << 21) + rng.integers(0, 1 << 21, int(cnt)) for bin_, cnt in parts if cnt])
    return from_bits(rng.permutation(b))


def bin_edges(n, below, low_bits, seed):
    """`below` values under an edge E and n - below from E on, E - 1 and E themselves among them:
    sorted[below - 1] has its low `low_bits` bits all 1 and sorted[below] all 0. low_bits = 21:
    a digit-1 bin edge (E = 1.0); 10: a digit-2 edge inside the bin of 1.0."""
    rng = np.random.default_rng(seed)
    E = (BIN_ONE << 21) + ((5 << 10) if low_bits == 10 else 0)
    span = 1 << (low_bits + 2)
    lo = E - 1 - rng.integers(0, span, below)
    hi = E + rng.integers(0, span, n - below)
    lo[0], hi[0] = E - 1, E
    return from_bits(rng.permutation(np.concatenate([lo, hi])))


def cap(C, n, k, pos, seed):
    """Exactly C values in the bin of the k-th smallest, which is the pos-th of them; the rest
    spread over 24 other bins on both sides."""
    rng = np.random.default_rng(seed)
    n_lo = k - pos
    n_hi = n - C - n_lo
    assert 0 <= pos < C and n_lo >= 0 and n_hi >= 0
    lo = ((BIN_ONE - 1 - rng.integers(0, 12, n_lo)) << 21) + rng.integers(0, 1 << 21, n_lo)
    hi = ((BIN_ONE + 1 + rng.integers(0, 12, n_hi)) << 21) + rng.integers(0, 1 << 21, n_hi)
    mid = (BIN_ONE << 21) + rng.integers(0, 1 << 21, C)
    return from_bits(rng.permutation(np.concatenate([lo, mid, hi])))


def check(ctx, steps, counts, ratios, variants, active=None, what=""):
    """One run against the reference; returns (got, want)."""
    want = sr.run_steps(steps, counts, ratios, variants, active)
    got = ctx.test_select(steps, counts, ratios, variants, active)
    sr.assert_equal(got, want, f"{what} variants {list(variants)}")
    return got, want


# ------------------------------------------------------------------ 1. sizes ----------------
SIZES = (1, 2, 255, 4095, 4096, 4097, 8193, 65535, 65536, 65537)


@functools.lru_cache(maxsize=None)
def sizes_case(n):
    """One pair per ratio, two steps of fresh distances (the second runs on what the first left)."""
    counts = [n] * len(RATIOS)
    steps = [np.concatenate([spread(n, 1000 * s + 10 * n + p) for p in range(len(RATIOS))]) for s in range(2)]
    for a in steps:
        a.setflags(write=False)
    return steps, counts


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, L, n, variant):
    steps, counts = sizes_case(n)
    if variant == 5 and n > 65536:
        with pytest.raises(L.AicpError) as e:
            ctx.test_select(steps, counts, RATIOS, [5, 5])
        assert e.value.code == L.AICP_ERR_INVALID
        return
    check(ctx, steps, counts, RATIOS, [variant, variant], what=f"n {n}")


def test_rejected_calls(ctx, L):
    d = spread(100, 1)
    bad = [
        dict(d2_steps=[d], counts=[100], ratios=[1.5], variants=[1]),
        dict(d2_steps=[d], counts=[100], ratios=[-0.1], variants=[1]),
        dict(d2_steps=[d], counts=[100], ratios=[np.nan], variants=[1]),
        dict(d2_steps=[d], counts=[100, 0], ratios=[0.5, 0.5], variants=[1]),
        dict(d2_steps=[d], counts=[100], ratios=[0.5], variants=[6]),
        dict(d2_steps=[d], counts=[100], ratios=[0.5], variants=[-1]),
        dict(d2_steps=[np.zeros(4097, np.float32)], counts=[1] * 4097, ratios=[0.5] * 4097, variants=[1]),
        dict(d2_steps=[], counts=[100], ratios=[0.5], variants=[]),
    ]
    for kw in bad:
        with pytest.raises(L.AicpError) as e:
            ctx.test_select(**kw)
        assert e.value.code == L.AICP_ERR_INVALID, kw["counts"][:2]
    # null pointers, through the C entry itself
    import ctypes as C

    cnt, rat, var = (C.c_uint32 * 1)(100), (C.c_float * 1)(0.5), (C.c_int32 * 1)(1)
    o_f, o_i, o_u, dirty = (C.c_float * 1)(), (C.c_int32 * 1)(), (C.c_uint32 * 1)(), C.c_uint64()
    dp = d.ctypes.data_as(C.POINTER(C.c_float))
    good = [ctx.h, 1, cnt, rat, None, 1, var, dp, o_f, o_i, o_i, o_u, o_u, C.byref(dirty)]
    for i in (0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13):
        args = list(good)
        args[i] = None
        assert L.lib.aicp_hip_test_select(*args) == L.AICP_ERR_INVALID, i
    for i, v in ((1, 0), (1, 4097), (5, 0)):  # no pair, more than kMaxPairs pairs, no step
        args = list(good)
        args[i] = v
        assert L.lib.aicp_hip_test_select(*args) == L.AICP_ERR_INVALID, (i, v)
    assert L.lib.aicp_hip_test_select(*good) == L.AICP_OK and dirty.value == 0
    check(ctx, [d], [100], [0.5], [1], what="after the rejected calls")


# ------------------------------------------------------------------ 2. candidate caps -------
CAPS = (2048, 2049, 8192, 8193, 12288, 12289)  # each template's LDS capacity and one more


@functools.lru_cache(maxsize=None)
def caps_case(C):
    n, ratio = 65536, 0.5
    k = sr.kth_index(n, ratio)
    pos = (0, C // 2, C - 1)
    steps = [np.concatenate([cap(C, n, k, p, 7 * C + i) for i, p in enumerate(pos)])]
    steps[0].setflags(write=False)
    # the construction: the k-th value's bin holds exactly C values in every pair
    for i in range(3):
        lim, _ = sr.select_one(steps[0][i * n:(i + 1) * n], ratio)
        assert sr.bin1(lim) == BIN_ONE
        assert int(np.sum(steps[0][i * n:(i + 1) * n].view(np.uint32) >> 21 == BIN_ONE)) == C
    return steps, [n] * 3, [ratio] * 3


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("C", CAPS)
def test_candidate_caps(ctx, C, variant):
    steps, counts, ratios = caps_case(C)
    # twice: the second select starts from what the first left (for the fused ones, a hit)
    check(ctx, steps * 2, counts, ratios, [variant, variant], what=f"cap {C}")


@pytest.mark.parametrize("variant", ALL)
def test_one_bin_and_one_value(ctx, variant):
    n = 20000
    ratios = [0.0, 0.358818, 0.7, 1.0]
    counts = [n] * 4
    a = np.concatenate([one_bin(n, 3 + p) for p in range(4)])
    b = np.concatenate([one_value(n) for _ in range(4)])
    check(ctx, [a, b, b], counts, ratios, [variant] * 3, what="one_bin, one_value")


@pytest.mark.parametrize("variant", ALL)
def test_zeros_and_denormals(ctx, variant):
    n = 10000
    d = zeros(n, 11)
    ratios = [0.2, 0.402, 0.9]  # the k-th among the zeros, among the denormals, among the normal numbers
    lims = [sr.select_one(d, r)[0] for r in ratios]
    assert lims[0] == 0.0 and 0 < lims[1] < np.finfo(np.float32).tiny and lims[2] > 1e-9
    check(ctx, [np.tile(d, 3)] * 2, [n] * 3, ratios, [variant] * 2, what="zeros")


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("low_bits", [21, 10])
def test_bin_edges(ctx, low_bits, variant):
    """Ranks k - 1, k and k + 1 straddle a digit-1 (or digit-2) bin edge, on either side."""
    n, ratio = 9000, 0.358818
    k = sr.kth_index(n, ratio)
    belows = (k, k + 1)  # sorted[k] = E (first of its bin) / sorted[k] = E - 1 (last of its bin)
    d = np.concatenate([bin_edges(n, b, low_bits, 5 + i) for i, b in enumerate(belows)])
    E = (BIN_ONE << 21) + ((5 << 10) if low_bits == 10 else 0)
    assert sr.select_one(d[:n], ratio)[0].view(np.uint32) == E
    assert sr.select_one(d[n:], ratio)[0].view(np.uint32) == E - 1
    check(ctx, [d, d], [n, n], [ratio, ratio], [variant] * 2, what=f"edge of the low {low_bits} bits")


# ------------------------------------------------------------------ 3. forced misses --------
A, B_LO, B_HI = BIN_ONE, BIN_ONE - 9, BIN_ONE + 6


def miss_cases(n):
    """name -> (step 0 distances with the k-th in bin A, step 1 distances with it elsewhere, ratio)."""
    k = sr.kth_index(n, 0.5)
    return {
        # the guessed bin is empty in the new distances
        "empty": (in_bins([(A, n)], 1), in_bins([(B_LO, n // 2 + 1), (B_HI, n - n // 2 - 1)], 2), 0.5),
        # the guessed bin holds 90 % of them: a large candidate count to discard
        "crowded": (in_bins([(A, n)], 3), in_bins([(A, n * 9 // 10), (B_HI, n - n * 9 // 10)], 4), 0.95),
        # the k-th value's bin holds more than any template keeps in LDS (n = 20000: 19900; a
        # single block: more than kHistBins)
        "spill": (in_bins([(A, n)], 5), in_bins([(B_LO, n - 100), (A, 100)], 6), 0.5),
        # the neighbouring bin, up and down
        "up": (bin_edges(n, k + 1, 21, 7), bin_edges(n, k, 21, 8), 0.5),
        "down": (in_bins([(A, n)], 9), bin_edges(n, k + 1, 21, 10), 0.5),
        # bin 0: the limit becomes 0.0
        "to_zero": (in_bins([(A, n)], 11), zeros(n, 12), 0.2),
    }


@pytest.mark.parametrize("variant", FUSED)
@pytest.mark.parametrize("name", ["empty", "crowded", "spill", "up", "down", "to_zero"])
@pytest.mark.parametrize("n", [3000, 20000])  # one block (the missing workgroup is the only one), several
def test_forced_miss(ctx, n, name, variant):
    d0, d1, ratio = miss_cases(n)[name]
    # a miss, a hit on the same distances, a miss back to the first bin, a hit
    steps, variants = [d0, d1, d1, d0, d0], [1] + [variant] * 4
    got, want = check(ctx, steps, [n], [ratio], variants, what=f"miss {name} n {n}")
    assert want["miss"][:, 0].tolist() == [0, 1, 1, 2, 2]  # (the construction)
    if name == "to_zero":
        assert got["limit"][1, 0] == 0.0 and got["b1"][1, 0] == 0


@pytest.mark.parametrize("variant", FUSED)
@pytest.mark.parametrize("n", [3000, 20000])
def test_fused_first_step(ctx, n, variant):
    """The guess of a fused select that runs first is k_init_state's 0: a miss unless the k-th
    value lies in bin 0."""
    d = np.concatenate([spread(n, 21), zeros(n, 22)])
    got, want = check(ctx, [d, d], [n, n], [0.7, 0.2], [variant] * 2, what="fused first")
    assert want["miss"].tolist() == [[1, 0], [1, 0]]


# ------------------------------------------------------------------ 4. several pairs --------
RAGGED = ([1, 4097, 60000, 300, 12289], [0.9, 0.358818, 0.7, 0.0, 1.0])
EQUAL = ([4096] * 6, [0.1, 0.25, 0.5, 0.7, float(NEAR_ONE), 1.0])


@functools.lru_cache(maxsize=None)
def batch_case(which):
    counts, ratios = RAGGED if which == "ragged" else EQUAL
    steps = [np.concatenate([spread(c, 100 * s + p) if p != 4 else one_bin(c, 100 * s + p)
                             for p, c in enumerate(counts)]) for s in range(2)]
    for a in steps:
        a.setflags(write=False)
    return steps, counts, ratios


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("which", ["ragged", "equal"])
def test_several_pairs(ctx, which, variant):
    steps, counts, ratios = batch_case(which)
    check(ctx, steps, counts, ratios, [variant] * 2, what=which)


# ------------------------------------------------------------------ 5. stopping, inactivity -
COUNTS4 = [5000, 3000, 4097, 9000]
RATIOS4 = [0.5, 0.7, 0.25, 0.358818]


def four_pairs(seed, all_inf=()):
    parts = [spread(c, seed + p) for p, c in enumerate(COUNTS4)]
    for p in all_inf:
        parts[p][:] = np.inf
    return np.concatenate(parts)


SEQUENCES = [[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [1, 2, 2]]


@pytest.mark.parametrize("variants", SEQUENCES, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("layout", ["middle", "last", "all"])
def test_stopping_and_inactive_pairs(ctx, layout, variants):
    """A pair without a finite distance stops (status 1) inside the select and stays as it was,
    although the later steps give it finite distances; a pair that starts inactive keeps its
    initial values; the other pairs of the launch are exact at every step."""
    if layout == "middle":  # pair 1 stops, pair 2 starts inactive
        stop, active = (1,), [1, 1, 0, 1]
    elif layout == "last":  # the stopping pair is the batch's last
        stop, active = (3,), [1, 0, 1, 1]
    else:  # every pair stops at step 0
        stop, active = (0, 1, 2, 3), [1, 1, 1, 1]
    steps = [four_pairs(40, all_inf=stop)] + [four_pairs(50 + s) for s in range(1, len(variants))]
    got, want = check(ctx, steps, COUNTS4, RATIOS4, variants, active, what=layout)
    for p in range(4):  # (the construction)
        if p in stop:
            assert want["status"][:, p].tolist() == [1] * len(variants) and not want["n_finite"][:, p].any()
        elif not active[p]:
            assert not any(want[key][:, p].any() for key in want)
        else:
            assert want["n_finite"][-1, p] > 0 and want["limit"][-1, p] > 0


# ------------------------------------------------------------------ 6. re-use ---------------
def test_context_reuse_after_test_select(ctx, L):
    """The entry leaves the context's shared buffers as the other calls expect them: after it,
    dists_quantile and a small align_batch give what a fresh context gives."""
    d = spread(30000, 77)
    pr = sy.make_pair(4000, 4000, seed=7)
    pairs = [dict(ref=pr.ref, read=pr.read, ref_origin=pr.ref_origin, read_origin=pr.read_origin)]
    flags = L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP
    res = float(np.float32(0.2))
    fresh = L.Context(0)
    try:
        q0 = fresh.dists_quantile(d, 0.7)
        T0, s0, rc0 = fresh.align_batch(pairs, flags=flags, resolution=res)
    finally:
        fresh.close()
    steps, counts, ratios = batch_case("ragged")
    for _ in range(2):
        for variant in ALL:
            check(ctx, steps, counts, ratios, [variant] * 2, what="re-use")
    q1 = ctx.dists_quantile(d, 0.7)
    T1, s1, rc1 = ctx.align_batch(pairs, flags=flags, resolution=res)
    assert np.float32(q0).view(np.uint32) == np.float32(q1).view(np.uint32)
    assert q1 == sr.select_one(d, 0.7)[0]
    assert rc0 == rc1 == 0
    np.testing.assert_array_equal(T0, T1)
    assert s0 == s1
    check(ctx, steps, counts, ratios, [1, 2], what="after align_batch")
