"""The numpy reference of the trimmed-limit select (select_reference.py) against brute force and
against the CPU oracle's getDistsQuantile. No GPU needed."""
import numpy as np
import pytest

import select_reference as sr


def brute(d2, ratio):
    """The k-th smallest finite value by counting, no sort: the value v with
    #(f < v) <= k < #(f <= v)."""
    f = [float(x) for x in d2 if x != np.inf]
    n = len(f)
    if n == 0:
        return None, 0
    k = sr.kth_index(n, ratio)
    for v in f:
        if sum(x < v for x in f) <= k < sum(x <= v for x in f):
            return np.float32(v), n
    raise AssertionError("no k-th value")


@pytest.mark.parametrize("seed", range(6))
def test_select_one_is_the_kth_smallest_finite(seed):
    rng = np.random.default_rng(seed)
    for n in (1, 2, 3, 10, 57):
        d2 = (rng.exponential(size=n) ** 3).astype(np.float32)
        d2[rng.random(n) < 0.2] = np.inf
        d2[rng.random(n) < 0.2] = 0.0
        if n > 5:
            d2[1:4] = d2[0]  # ties
        for ratio in (0.0, 0.25, 0.358818, 0.7, np.nextafter(np.float32(1), np.float32(0)), 1.0):
            got, want = sr.select_one(d2, ratio), brute(d2, ratio)
            assert got[1] == want[1]
            if want[0] is None:
                assert got[0] is None
            else:
                assert np.float32(got[0]).view(np.uint32) == want[0].view(np.uint32)


def test_k_is_a_float32_product():
    # float32(0.7) = 0.699999988...: 10 times it is 6.99999988 exactly, which rounds to 7.0f as a
    # float32 product and stays below 7 as a double product of the same two floats
    assert sr.kth_index(10, 0.7) == 7
    assert int(10.0 * float(np.float32(0.7))) == 6
    d2 = np.arange(10, dtype=np.float32)
    assert sr.select_one(d2, 0.7) == (7.0, 10)
    assert sr.kth_index(10, 1.0) == 9
    assert sr.kth_index(1, 0.0) == 0
    # a ratio just below 1 on a count whose product rounds up to n: clamped to the last rank
    assert sr.kth_index(65536, np.nextafter(np.float32(1), np.float32(0))) == 65535


def test_contract_rejects_nan_and_negative_zero():
    for bad in (np.nan, -0.0, -1.0):
        with pytest.raises(AssertionError):
            sr.select_one(np.array([1.0, bad], np.float32), 0.5)
    assert sr.select_one(np.array([0.0, 1e-45, np.inf], np.float32), 1.0) == (np.float32(1e-45), 2)


def quantile_exact_input(n):
    """test_gpu_parity.py::test_quantile_exact's distances."""
    rng = np.random.default_rng(n)
    d2 = rng.exponential(size=n).astype(np.float32) ** 3
    if n > 10:
        d2[::13] = np.inf
        d2[3 : n // 3] = d2[2]  # heavy ties
    return d2


@pytest.mark.parametrize("n", [1, 7, 1000, 131071, 500000])
def test_reference_equals_oracle_on_quantile_exact_inputs(oracle, n):
    d2 = quantile_exact_input(n)
    for q in (0.25, 0.358818, 0.5, 0.7, 1.0):
        ref, err = oracle.dists_quantile(d2, q)
        assert err == 0
        limit, nf = sr.select_one(d2, q)
        assert nf == int(np.sum(d2 != np.inf))
        assert np.float32(limit).view(np.uint32) == np.float32(ref).view(np.uint32)
    assert oracle.dists_quantile(np.full(10, np.inf, np.float32), 0.5)[1] != 0
    assert sr.select_one(np.full(10, np.inf, np.float32), 0.5) == (None, 0)


def test_run_steps_state_rules():
    """Frozen outputs of stopped and inactive pairs, and the miss count of fused steps."""
    counts = [4, 3, 2]
    a = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.float32)
    b = a.copy()
    b[4:7] = np.inf  # pair 1 stops at step 1
    c = a * 1024  # other digit-1 bins
    out = sr.run_steps([a, b, c, c], counts, [0.5, 0.5, 1.0], [1, 2, 2, 4], active=[1, 1, 0])
    # pair 0: k = 2 of 4
    np.testing.assert_array_equal(out["limit"][:, 0], [3, 3, 3072, 3072])
    np.testing.assert_array_equal(out["miss"][:, 0], [0, 0, 1, 1])  # step 0 is not fused; step 1 hits
    # pair 1: k = 1 of 3, then stopped: everything but the status stays
    np.testing.assert_array_equal(out["limit"][:, 1], [6, 6, 6, 6])
    np.testing.assert_array_equal(out["status"][:, 1], [0, 1, 1, 1])
    np.testing.assert_array_equal(out["n_finite"][:, 1], [3, 3, 3, 3])
    np.testing.assert_array_equal(out["miss"][:, 1], [0, 0, 0, 0])
    # pair 2: never active
    for key in out:
        assert not out[key][:, 2].any()
    # a fused first step guesses bin 0
    out = sr.run_steps([a, np.zeros(9, np.float32)], [9], [0.5], [2, 3])
    np.testing.assert_array_equal(out["miss"][:, 0], [1, 2])
    np.testing.assert_array_equal(out["b1"][:, 0], [sr.bin1(5.0), 0])
