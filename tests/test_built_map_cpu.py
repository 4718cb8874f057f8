"""App's built-map localization stream without a device: the host restatement
(tests/built_map_reference.py) on the shared fixture, aicp_hip_built_map_window against a
brute-force simulation of App's counter, the C structs' layout, and the argument checks that need
no device. The GPU side is tests/test_built_map_stream.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import built_map_reference as br


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def world(oracle):
    first = br.make_first_cloud(oracle)
    reads, poses, origins = br.make_stream()
    return first, reads, poses, origins


EXPECT = {
    False: dict(accepted=[1, 1, 1, 1, 0, 1, 1, 1, 1, 1], refs=[2, 6, 9], iters=[9, 6, 6, 8, 10, 7, 6, 6, 6, 6],
                map_points=[59522] * 3 + [62522] * 4 + [65522] * 3),
    True: dict(accepted=[1] * 10, refs=[2, 5, 8], iters=[9, 6, 4, 4, 5, 5, 4, 4, 4, 5],
               map_points=[59522] * 3 + [62522] * 3 + [65522] * 3 + [68522]),
}


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_replay_patterns(oracle, world, L, debug):
    """The free-running replay on the fixture. Robot mode: reading 4 (the jump) is dropped, the
    3rd, 6th and 9th accepted readings become references. Debug mode: reading 4 is moved by
    initialT_ first, so its correction is small and it is accepted. Every registration settles
    below the iteration limit (one that never settles amplifies rounding differences)."""
    first, reads, poses, origins = world
    assert first.shape == (59522, 3) and all(r.shape == (3000, 3) for r in reads)
    rec, final = br.replay(oracle, first, reads, poses, origins, debug=debug, **br.PARAMS)
    e = EXPECT[debug]
    assert [r["status"] for r in rec] == [0] * 10
    assert [r["accepted"] for r in rec] == e["accepted"]
    assert [i for i, r in enumerate(rec) if r["is_reference"]] == e["refs"]
    assert [r["stats"].iterations for r in rec] == e["iters"]
    assert max(r["stats"].iterations for r in rec) < oracle.default_config().max_iter
    assert [r["map_points"] for r in rec] == e["map_points"] and len(final) == 68522
    np.testing.assert_array_equal(final[:len(first)], first)  # the map only grows at its tail
    assert all(16000 <= r["crop_points"] <= 21000 for r in rec), [r["crop_points"] for r in rec]
    # no ratio is clamped: every overlap is inside the auto-tune's open range
    assert all(25.0 < r["overlap"] < 70.0 for r in rec), [r["overlap"] for r in rec]
    assert all(r["ratio"] == np.float32(oracle.autotune_ratio(r["overlap"])) for r in rec)
    if not debug:
        assert 51.0 < rec[0]["overlap"] < 51.5 and 42.0 < min(r["overlap"] for r in rec) < 42.5
        assert 0.55 < abs(rec[4]["T"][1, 3]) < 0.75
        prm = L.default_built_map_params(reference_update_frequency=3)
        wins, changes, inside = br.simulate_windows(e["accepted"], 3, lambda a, rem: L.built_map_window(a, prm, rem))
        assert wins == [3, 3, 1, 3] and changes == e["refs"] and not inside


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_replay_jump_on_reading_0(oracle, world, debug):
    """getNbClouds() != 0 holds from the first reading on (the graph holds the first cloud), so
    the first reading is dropped when it carries the jump; a dropped reading changes nothing, so
    debug mode sees the same initialT_ = I for reading 1."""
    first = world[0]
    reads, poses, origins = br.make_stream(3, br.JUMP_ON_0)
    rec, final = br.replay(oracle, first, reads, poses, origins, debug=debug, **br.PARAMS)
    assert abs(rec[0]["T"][1, 3]) > 0.4
    assert [r["accepted"] for r in rec] == [0, 1, 1]
    assert not any(r["is_reference"] for r in rec) and len(final) == len(first)
    assert max(r["stats"].iterations for r in rec) < oracle.default_config().max_iter


def test_window_never_spans_a_map_change(L):
    """Every accept / drop sequence of length <= 8 for frequencies 1-5: no map change falls
    strictly inside a window, and the windows cover the stream."""
    for freq in range(1, 6):
        prm = L.default_built_map_params(reference_update_frequency=freq)
        window = lambda a, rem: L.built_map_window(a, prm, rem)
        for n in range(1, 9):
            for accept in itertools.product((0, 1), repeat=n):
                wins, changes, inside = br.simulate_windows(accept, freq, window)
                assert sum(wins) == n and not inside, (freq, accept, wins, changes, inside)
                if all(accept):  # every window ends exactly on a map change (but the last)
                    ends = list(np.cumsum(wins) - 1)
                    assert ends[:-1] == changes[:len(ends) - 1], (wins, changes)
                    assert all(w == freq for w in wins[:-1])
        dbg = L.default_built_map_params(reference_update_frequency=freq, debug=True)
        assert [L.built_map_window(a, dbg, 9) for a in range(freq)] == [1] * freq


def test_window_limits(L):
    prm = L.default_built_map_params()
    assert [L.built_map_window(a, prm, 100) for a in range(7)] == [5, 4, 3, 2, 1, 0, 0]  # acc >= frequency: 0
    assert L.built_map_window(0, prm, 2) == 2 and L.built_map_window(3, prm, 0) == 0
    big = L.default_built_map_params(reference_update_frequency=10000)
    assert L.built_map_window(0, big, 20000) == 4096 and L.built_map_window(9000, big, 20000) == 1000
    for bad in (dict(reference_update_frequency=0), dict(reference_update_frequency=-2), dict(flags=16),
                dict(flags=2), dict(max_correction_magnitude=float("nan")), dict(resolution=0.0),
                dict(resolution=float("nan"))):
        assert L.built_map_window(0, L.default_built_map_params(**bad), 5) == 0, bad
    assert L.built_map_window(0, L.default_built_map_params(resolution=0.0, overlap=False), 5) == 5
    assert L.lib.aicp_hip_built_map_window(0, None, 5) == 0


def test_struct_sizes_and_defaults(L):
    assert C.sizeof(L.BuiltMapParams) == 32
    assert sum(C.sizeof(t) for _, t in L.BuiltMapParams._fields_) == 32  # no implicit padding
    assert L.BuiltMapParams.resolution.offset == 16 and L.BuiltMapParams.flags.offset == 24
    assert C.sizeof(L.BuiltMapResult) == 128
    assert sum(C.sizeof(t) for _, t in L.BuiltMapResult._fields_) == 128
    assert L.BuiltMapResult.map_points.offset == 16 and L.BuiltMapResult.icp.offset == 56
    assert C.sizeof(L.IcpStats) == 72
    assert C.sizeof(L.BuiltMapTiming) == 24
    assert sum(C.sizeof(t) for _, t in L.BuiltMapTiming._fields_) == 24
    p = L.default_built_map_params()
    assert (p.reference_update_frequency, p.max_correction_magnitude, p.crop_min, p.crop_max, p.resolution, p.flags,
            p.pad) == (5, 1.0, -15.0, 15.0, 0.2, L.AICP_RUN_OVERLAP, 0)
    q = L.default_built_map_params(overlap=False, debug=True, time_nn=True)
    assert q.flags == L.AICP_SEQ_DEBUG | L.AICP_RUN_TIME_NN
    with pytest.raises(AttributeError):
        L.default_built_map_params(map_refilter_every=3)


def test_invalid_arguments_need_no_device(L):
    done = C.c_size_t(7)
    assert L.lib.aicp_hip_built_map_sequence_run(None, None, None, None, None, None, 0, None, None,
                                                 C.byref(done)) == L.AICP_ERR_INVALID
    assert L.lib.aicp_hip_built_map_sequence_run(None, None, None, None, None, None, 0, None, None,
                                                 None) == L.AICP_ERR_INVALID
    assert L.lib.aicp_hip_map_align_batch(None, None, None, -1.0, 1.0, None, None, 0, 0.2, 0, None,
                                          None) == L.AICP_ERR_INVALID
    t = L.BuiltMapTiming()
    assert L.lib.aicp_hip_last_built_map_timing(None, C.byref(t)) == L.AICP_ERR_INVALID
    n = C.c_size_t()
    assert L.lib.aicp_hip_map_capacity(None, C.byref(n)) == L.AICP_ERR_INVALID
