"""The sweep accumulator on the device (aicp_hip_accum_*, kernels_accum.hip) against the numpy
restatement of tests/accumulator_reference.py, and its pre-filter bridge against the composition of
the existing calls it replaces. Every comparison is exact: same points, same order, same bits."""
import numpy as np
import pytest

import accumulator_reference as ar
from aicp_mapping_amd import synthetic as sy

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)  # the wave, tile and multi-tile edges


@pytest.fixture(scope="module")
def ctx():
    import aicp_mapping_amd._lib as L

    c = L.Context(0)
    yield c
    c.close()


def specials():
    """5 non-finite points, and per axis and side one point exactly on the cube's face (kept) and
    one at nextafter beyond it (dropped): 17 rows."""
    rows = [(np.nan, 1.0, 2.0), (3.0, np.inf, -4.0), (5.0, 6.0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, 0.0, np.nan)]
    for k in range(3):
        for s in (-1.0, 1.0):
            on = np.array([7.5, -11.25, 2.125], F)
            off = on.copy()
            on[k] = F(s * 30.0)
            off[k] = np.nextafter(F(s * 30.0), F(s * np.inf))
            rows += [tuple(on), tuple(off)]
    return np.array(rows, F)


def make_sweep(n, seed):
    """n points uniform in +-40 m (about 42 % survive the +-30 m cube), with the 17 special rows at
    random places (as many of them as the sweep has room for, the on-face points first)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-40.0, 40.0, (n, 3)).astype(F)
    sp = specials()
    sp = sp[np.r_[5:17, 0:5]][:n] if n < len(sp) else sp
    if n:
        p[rng.choice(n, len(sp), replace=False)] = sp
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_reference(sweeps, poses, batch_size):
    acc = ar.Accumulator(batch_size=batch_size)
    for s, P in zip(sweeps, poses):
        acc.push(s, P)
    return acc


def check(acc, ref):
    assert acc.counter == ref.counter and acc.finished == ref.finished
    assert np.array_equal(acc.kept_per_sweep(), ref.kept_per_sweep())
    assert len(acc) == len(ref.cloud)
    assert same_bits(acc.getCloud(), ref.cloud)


@pytest.mark.parametrize("n", SIZES)
def test_one_sweep_equals_the_reference(ctx, n):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    s, P = make_sweep(n, 100 + n), ar.general_pose()
    ref = run_reference([s], [P], 1)
    if n >= 17:
        assert (~np.isfinite(s).all(axis=1)).sum() == 5
        assert ref.kept[0] >= 6 + (n >= 1023) * 0.35 * n and n - ref.kept[0] >= 11 + (n >= 1023) * 0.5 * n
    acc = SweepAccumulator(ctx, max(n, 1), batch_size=1)
    acc.push(s, P)
    check(acc, ref)
    assert acc.finished
    acc.free()


def test_mixed_sizes_finish_ignore_clear_and_reuse(ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    poses = [ar.general_pose(), ar.general_pose(-120.0, 3.0, -9.0, (-3.0, 40.0, 2.0)),
             ar.general_pose(171.0, -2.0, 1.0, (0.25, 0.5, -0.75))]
    sweeps = [make_sweep(n, 7 + n) for n in (1025, 0, 700)]
    acc = SweepAccumulator(ctx, 4000, batch_size=3)
    assert acc.counter == 0 and not acc.finished and len(acc) == 0 and len(acc.getCloud()) == 0
    for i, (s, P) in enumerate(zip(sweeps, poses)):
        assert not acc.finished
        acc.push(s, P)
        assert acc.counter == i + 1
    ref = run_reference(sweeps, poses, 3)
    assert acc.finished
    check(acc, ref)
    acc.push(make_sweep(300, 1), poses[0])  # if (finished_) return;
    check(acc, ref)
    acc.clear()
    assert acc.counter == 0 and not acc.finished and len(acc) == 0 and not acc.kept_per_sweep().any()
    assert len(acc.getCloud()) == 0
    # a second reading through the same handle: the tail starts at zero again
    sweeps2 = [make_sweep(n, 900 + n) for n in (333, 1500, 64)]
    for s, P in zip(sweeps2, poses[::-1]):
        acc.push(s, P)
    check(acc, run_reference(sweeps2, poses[::-1], 3))
    acc.free()


def test_all_dropped_and_all_kept_sweeps(ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    rng = np.random.default_rng(5)
    out = rng.uniform(30.5, 90.0, (1300, 3)).astype(F) * rng.choice([-1.0, 1.0], (1300, 1)).astype(F)
    out[::7] = np.nan
    inside = rng.uniform(-30.0, 30.0, (2049, 3)).astype(F)
    sweeps = [make_sweep(1100, 1), out, make_sweep(900, 2), inside]
    poses = [ar.general_pose(10.0 * i, -i, 2.0 * i, (i, -2.0 * i, 0.1 * i)) for i in range(4)]
    ref = run_reference(sweeps, poses, 4)
    assert ref.kept[1] == 0 and ref.kept[3] == 2049 and ref.kept[0] and ref.kept[2]
    acc = SweepAccumulator(ctx, sum(len(s) for s in sweeps), batch_size=4)
    for s, P in zip(sweeps, poses):
        acc.push(s, P)
    check(acc, ref)
    acc.free()


def test_row_strides_give_the_same_cloud(ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    sweeps = [make_sweep(n, 40 + n) for n in (1025, 513)]
    poses = [ar.general_pose(), ar.general_pose(-20.0, 6.0, 3.0, (1.0, 2.0, 3.0))]
    ref = run_reference(sweeps, poses, 2)
    for w in (3, 4, 8):  # rows of 12, 16 and 32 bytes; what follows xyz in a row is not read
        acc = SweepAccumulator(ctx, 1538, batch_size=2)
        for s, P in zip(sweeps, poses):
            rows = np.full((len(s), w), np.nan, F)
            rows[:, :3] = s
            acc.push(rows, P)
        check(acc, ref)
        acc.free()


def test_capacity_is_an_upper_bound_on_the_pushed_points(ctx):
    import aicp_mapping_amd._lib as L
    from aicp_mapping_amd.accumulator import SweepAccumulator

    P = ar.general_pose()
    a, b, c = make_sweep(1000, 1), make_sweep(501, 2), make_sweep(500, 3)
    acc = SweepAccumulator(ctx, 1500, batch_size=4)
    acc.push(a, P)
    before = (acc.counter, acc.finished, len(acc), acc.kept_per_sweep(), acc.getCloud())
    with pytest.raises(L.AicpError) as e:  # 1501 > 1500, whatever the crop would keep
        acc.push(b, P)
    assert e.value.code == L.AICP_ERR_INVALID
    after = (acc.counter, acc.finished, len(acc), acc.kept_per_sweep(), acc.getCloud())
    assert before[:3] == after[:3] and np.array_equal(before[3], after[3]) and same_bits(before[4], after[4])
    acc.push(c, P)  # fits exactly
    check(acc, run_reference([a, c], [P, P], 4))
    with pytest.raises(L.AicpError) as e:
        acc.push(make_sweep(1, 4), P)
    assert e.value.code == L.AICP_ERR_INVALID
    acc.push(np.zeros((0, 3), F), P)  # an empty sweep still fits, and counts
    assert acc.counter == 3
    acc.free()


def test_push_has_staged_the_rows_when_it_returns(ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    sweeps = [make_sweep(1025, 500 + i) for i in range(16)]
    poses = [ar.general_pose(3.0 * i, 0.5 * i, -0.25 * i, (0.5 * i, 0.1 * i, 0.0)) for i in range(16)]
    ref = run_reference(sweeps, poses, 16)
    acc = SweepAccumulator(ctx, 16 * 1025, batch_size=16)
    buf = np.empty((1025, 3), F)
    for s, P in zip(sweeps, poses):
        buf[:] = s
        acc.push(buf, P)
        buf[:] = 12.5  # inside the cube: a late read of the caller's buffer would show
    check(acc, ref)
    acc.free()


def test_sweeps_larger_than_the_first_staging_area(ctx):
    """The staging area and the pinned slots start at 65536 rows and grow with the sweeps, while
    earlier sweeps are still in flight."""
    from aicp_mapping_amd.accumulator import SweepAccumulator

    sizes = (1025, 70000, 300, 100000, 65537)
    sweeps = [make_sweep(n, 60 + i) for i, n in enumerate(sizes)]
    poses = [ar.general_pose(-15.0 * i, 2.0, -1.0, (0.3 * i, 1.0, -0.2 * i)) for i in range(len(sizes))]
    acc = SweepAccumulator(ctx, sum(sizes), batch_size=len(sizes))
    for s, P in zip(sweeps, poses):
        acc.push(s, P)
    check(acc, run_reference(sweeps, poses, len(sizes)))
    acc.free()


@pytest.fixture(scope="module")
def bridge(ctx):
    from aicp_mapping_amd.accumulator import SweepAccumulator

    sweeps, poses = ar.bridge_sweeps()
    acc = SweepAccumulator(ctx, sum(len(s) for s in sweeps), batch_size=3)
    for s, P in zip(sweeps, poses):
        acc.push(s, P)
    ref = run_reference(sweeps, poses, 3)
    check(acc, ref)
    yield acc, ref
    acc.free()


BRIDGE_T = sy.make_T(4.0, -1.0, 0.5, (0.3, -0.2, 0.1)).astype(F)


@pytest.mark.parametrize("moved", (False, True))
def test_prefilter_bridge_equals_the_composition(ctx, bridge, moved):
    acc, ref = bridge
    T = BRIDGE_T if moved else None
    got = acc.prefilter(T)
    st = ctx.last_prefilter_stats()
    assert st["knn_queries"] > 0 and st["device_ms"] > 0 and st["wall_ms"] >= st["device_ms"]
    cloud = acc.getCloud()
    exp = ctx.prefilter(ctx.transform(T, cloud) if moved else cloud)
    assert len(exp) >= 50 and same_bits(got, exp)
    check(acc, ref)  # the accumulator keeps its cloud


def test_bridge_output_registers_as_the_composition_does(ctx, bridge):
    acc, _ = bridge
    got = acc.prefilter()
    exp = ctx.prefilter(acc.getCloud())
    second = ctx.prefilter(sy.sample_scene(sy.make_scene(7), np.random.default_rng(21), (0.15, 0.1, 0.7), half=3.0,
                                           spacing=0.05).astype(F))
    assert len(second) >= 50
    Tg, sg = ctx.register(second, got)
    Te, se = ctx.register(second, exp)
    assert same_bits(Tg, Te) and sg["iterations"] == se["iterations"] and sg["iterations"] > 0
