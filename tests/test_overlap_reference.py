"""The overlap's plain reference (overlap_reference.py) held to the C++ oracle and to itself (CPU).

Two independent transcriptions of octomap's computeRayKeys, the oracle's C++ and the module's
Python, agree on every ray of every case, key for key in order, and on every pair's counts and
percentage. Each case reaches, on the reference alone, the condition it exists for. The layout
model round-trips. The stream's host bound of a cloud's key-list words (key_bound, through the
host-only aicp_hip_test_key_bound) is an upper bound of the reference's totals, in its rigid form
under 24 rigid motions of cloud and origin, and not an absurd one.
"""
import numpy as np
import pytest

import overlap_reference as ov

f32 = np.float32
case_param = pytest.mark.parametrize("case", ov.CASES, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@case_param
def test_ray_keys_equal_the_oracle(oracle, case):
    R = ov.reference(case)
    for (pts, org), infos in zip(R.clouds, R.infos):
        o32 = np.asarray(org, np.float64).astype(np.float32)
        for p, info in zip(pts, infos):
            ks = oracle.ray_keys(o32, p, case.res)
            got = () if ks is None else tuple(ks.tolist())
            assert hash(got) == info["h"], (case.name, o32, p, len(got))


@case_param
def test_counts_and_percentage_equal_the_oracle(oracle, case):
    R = ov.reference(case)
    for p, (n, pc, _) in enumerate(ov.expected(case)):
        ref, ro = R.clouds[R.pair_group[p]]
        read, do = R.clouds[R.G + p]
        o_pc, o_cnt = oracle.overlap(ref, ro, read, do, case.res)
        assert tuple(int(c) for c in o_cnt) == n, (case.name, p)
        assert ov.same_f32(o_pc, pc), (case.name, p, o_pc, pc)


@case_param
def test_case_reaches_its_condition(case):
    case.cond(ov.reference(case))


def test_many_clouds_reach_every_end_bit():
    assert {ov.key_end_bit(n) for n in ov.MANY} == {49, 50, 51, 52}
    assert [ov.key_end_bit(n) for n in (1, 2, 3, 4, 7, 8)] == [49, 50, 50, 51, 51, 52]
    for n in ov.MANY:  # the pad tag n sorts after every cloud tag below the end bit
        assert n < 1 << (ov.key_end_bit(n) - 48)


def test_ratio_model_equals_the_oracle(oracle):
    for v in (0.0, 24.999, 25.0, 25.004, 33.3333, 47.12345, 69.996, 70.0, 70.5, 100.0):
        assert ov.same_f32(ov.autotune_ratio(f32(v)), oracle.autotune_ratio(float(f32(v)))), v


@pytest.mark.parametrize("seed", range(4))
def test_layout_round_trip(seed):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 65000, 3) if seed else np.array([0, 1, 65500])
    hi = np.minimum(lo + rng.integers(0, 40, 3), 65535)
    for k in range(3):
        mn, dim = ov.ovl_axis(int(lo[k]), int(hi[k]), ov.BRICK[k])
        assert mn % ov.BRICK[k] == 0 and dim % ov.BRICK[k] == 0
        assert mn <= lo[k] - 2 and mn + dim > hi[k] + 2  # two voxels of padding on both sides
        assert mn > lo[k] - 2 - ov.BRICK[k] and mn + dim <= hi[k] + 3 + ov.BRICK[k]  # and no brick to spare
    mn, dim = ov.ovl_desc(lo.tolist(), hi.tolist())
    S = {ov.pack(tuple(int(v) for v in rng.integers(lo, hi + 1))) for _ in range(500)}
    S |= {ov.pack(tuple(int(v) for v in lo)), ov.pack(tuple(int(v) for v in hi))}
    m = ov.encode_map(S, mn, dim)
    assert int(m.sum()) == len(S)  # ovl_index is injective on the box
    assert ov.decode_map(m, mn, dim) == S
    m[7] = 3
    with pytest.raises(AssertionError):
        ov.decode_map(m, mn, dim)
    assert ov.ovl_axis(ov.EMPTY_LO, ov.EMPTY_HI, 8) == ov.ovl_axis(0, 0, 8) == (-8, 16)


def _all_rays(R):
    O = np.concatenate([np.repeat(np.asarray(o, np.float64).astype(np.float32)[None], len(p), 0) for p, o in R.clouds])
    return O, np.concatenate([p for p, _ in R.clouds]), np.cumsum([0] + [len(p) for p, _ in R.clouds])


@case_param
def test_array_walk_equals_the_scalar_walk(case):
    R = ov.reference(case)
    O, P, _ = _all_rays(R)
    assert np.array_equal(ov.ray_counts(O, P, case.res), np.concatenate(R.counts))


def rigid_motions():
    """24 rigid motions: rotations about every axis and about diagonals, 45-degree ones included
    (they maximise sum |dk| for a given distance), each with a translation of up to 50 m."""
    rng = np.random.default_rng(5)
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 1)]
    out = []
    for i, a in enumerate(axes):
        a = np.array(a, np.float64) / np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        for ang in (np.pi / 4, np.pi / 2 if i % 2 else 3 * np.pi / 4, rng.uniform(0, 2 * np.pi)):
            Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
            t = rng.uniform(-1, 1, 3)
            out.append((Rm.astype(np.float32), (t / np.linalg.norm(t) * rng.uniform(0, 50)).astype(np.float32)))
    return out


def move(Rm, t, p):
    """aicp_hip_transform's float expression: ((T0 x + T1 y) + T2 z) + T3 per row"""
    p = np.asarray(p, np.float32)
    return np.stack([((Rm[r, 0] * p[:, 0] + Rm[r, 1] * p[:, 1]) + Rm[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)


@case_param
def test_key_bound_holds(L, case):
    R = ov.reference(case)
    for (pts, org), cnt in zip(R.clouds, R.counts):
        bound, cap = L.key_bound(pts, org, case.res, rigid=0)
        assert cap == 3 * 65536 + 8
        total, n_valid = int(cnt.sum()), int((cnt > 0).sum())
        assert bound >= total, (case.name, bound, total)
        assert bound <= len(pts) * cap
        if case.name in ov.ORDINARY:  # not an absurd bound
            assert bound <= 4 * total + 16 * len(pts), (case.name, bound, total)
        assert int(cnt.max(initial=0)) <= cap and n_valid <= len(pts)


@case_param
def test_rigid_key_bound_holds_under_rigid_motions(L, case):
    R = ov.reference(case)
    O, P, seg = _all_rays(R)
    bounds = [L.key_bound(pts, org, case.res, rigid=1)[0] for pts, org in R.clouds]
    for c, (b, cnt) in enumerate(zip(bounds, R.counts)):
        assert b >= int(cnt.sum()), (case.name, c)
        if case.name in ov.ORDINARY:
            assert b <= 4 * int(cnt.sum()) + 16 * len(cnt), (case.name, c, b, int(cnt.sum()))
    with np.errstate(all="ignore"):
        for m, (Rm, t) in enumerate(rigid_motions()):
            cnt = ov.ray_counts(move(Rm, t, O), move(Rm, t, P), case.res)
            for c, b in enumerate(bounds):
                total = int(cnt[seg[c]:seg[c + 1]].sum())
                assert b >= total, (case.name, "cloud", c, "motion", m, b, total)
