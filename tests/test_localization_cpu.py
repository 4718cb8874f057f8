"""App's localization stream without a device: the host restatement (tests/localization_reference.py)
on the shared fixture, aicp_hip_localization_window against a brute-force simulation of App's
counters, and the C structs' layout. The GPU side is tests/test_localization_stream.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import localization_reference as lr


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def world(oracle):
    mp = lr.make_map(oracle)
    reads, poses, origins = lr.make_stream(10, lr.JUMPS)
    return mp, reads, poses, origins


def test_fixture_map(world):
    mp = world[0]
    assert mp.shape == (59522, 3)


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_replay_patterns(oracle, world, L, debug):
    """The free-running replay on the fixture: readings 2 and 5 (the jumps) are dropped, the
    1st, 4th and 7th accepted readings merge (freq 3), the 1st and 5th re-filter (every 4)."""
    mp, reads, poses, origins = world
    rec, final = lr.replay(oracle, mp, reads, poses, origins, debug=debug, **lr.PARAMS)
    assert [r["status"] for r in rec] == [0] * 10
    assert [r["accepted"] for r in rec] == [1, 1, 0, 1, 1, 0, 1, 1, 1, 1]
    assert [i for i, r in enumerate(rec) if r["merged"]] == [0, 4, 8]
    assert [i for i, r in enumerate(rec) if r["refiltered"]] == [0, 6]
    assert all(17000 <= r["crop_points"] <= 19999 for r in rec), [r["crop_points"] for r in rec]
    t = np.array([np.abs(r["T"][:3, 3]) for r in rec])
    for i in (2, 5):
        assert 0.55 < t[i, 1] < 0.75, (i, t[i])
    ok = [i for i in range(1, 10) if i not in (2, 5)]
    assert t[ok].max() <= 0.33, t
    assert rec[0]["map_points"] == len(mp) and len(final) != len(mp)
    if not debug:  # the windows the accept pattern gives (robot mode)
        prm = L.default_localization_params(**lr.PARAMS)
        wins, changes, inside = lr.simulate_windows([r["accepted"] for r in rec], 3, 4, True,
                                                    lambda c, rem: L.localization_window(c, prm, rem))
        assert wins == [1, 3, 1, 1, 1, 2, 1] and changes == [0, 4, 6, 8] and not inside


@pytest.mark.parametrize("debug,accepted", [(False, [1, 1, 1]), (True, [1, 0, 0])], ids=["robot", "debug"])
def test_replay_jump_on_reading_0(oracle, world, debug, accepted):
    """The first processed cloud can never be dropped (getNbClouds() != 0, app.cpp:369): reading 0
    carries the jump, is accepted, merged and re-filtered. In debug mode its correction then moves
    the later readings by initialT_, away from where their crops were taken."""
    mp = world[0]
    reads, poses, origins = lr.make_stream(3, lr.JUMP_ON_0)
    rec, _ = lr.replay(oracle, mp, reads, poses, origins, debug=debug, **lr.PARAMS)
    assert abs(rec[0]["T"][1, 3]) > 0.4 and abs(abs(rec[0]["T"][1, 3]) - 0.70) < 0.05
    assert (rec[0]["accepted"], rec[0]["merged"], rec[0]["refiltered"]) == (1, 1, 1)
    assert [r["accepted"] for r in rec] == accepted


@pytest.mark.parametrize("freq,refilter,merge", list(itertools.product((1, 3, 5), (0, 4, 30), (True, False))))
def test_window_never_spans_a_map_change(L, freq, refilter, merge):
    prm = L.default_localization_params(reference_update_frequency=freq, map_refilter_every=refilter, merge=merge)
    rng = np.random.default_rng(100 * freq + refilter + (7 if merge else 0))
    window = lambda c, rem: L.localization_window(c, prm, rem)
    for trial in range(40):
        n = int(rng.integers(1, 90))
        accept = (rng.random(n) < rng.choice([0.5, 0.8, 1.0])).astype(int).tolist()
        wins, changes, inside = lr.simulate_windows(accept, freq, refilter, merge, window)
        assert sum(wins) == n and not inside, (accept, wins, changes, inside)
        if not merge:
            assert wins == [n] and not changes
        if all(accept) and merge:  # every window ends exactly on a map change (but the last)
            ends = list(np.cumsum(wins) - 1)
            assert ends[:-1] == changes[:len(ends) - 1], (wins, changes)
    dbg = L.default_localization_params(reference_update_frequency=freq, map_refilter_every=refilter, merge=merge,
                                        debug=True)
    assert [L.localization_window(c, dbg, 9) for c in range(12)] == [1] * 12


def test_window_limits(L):
    prm = L.default_localization_params(merge=False)
    assert L.localization_window(0, prm, 10000) == 4096
    assert L.localization_window(3, prm, 0) == 0
    bad = L.default_localization_params(reference_update_frequency=0)
    assert L.localization_window(0, bad, 5) == 0
    prm = L.default_localization_params()
    assert [L.localization_window(c, prm, 100) for c in range(7)] == [1, 5, 4, 3, 2, 1, 5]
    assert L.localization_window(26, prm, 100) == 5 and L.localization_window(28, prm, 100) == 3  # re-filter at 31


def test_struct_sizes_and_defaults(L):
    assert C.sizeof(L.LocalizationParams) == 24
    assert C.sizeof(L.LocalizationResult) == 128
    assert sum(C.sizeof(t) for _, t in L.LocalizationResult._fields_) == 128  # no implicit padding
    assert L.LocalizationResult.icp.offset == 56 and C.sizeof(L.IcpStats) == 72
    assert C.sizeof(L.LocalizationTiming) == 32
    p = L.default_localization_params()
    assert (p.reference_update_frequency, p.map_refilter_every, p.max_correction_magnitude, p.crop_min, p.crop_max,
            p.flags) == (5, 30, 1.0, -15.0, 15.0, L.AICP_LOC_MERGE)
    assert L.AICP_LOC_MERGE == 16 and not L.AICP_LOC_MERGE & (L.AICP_SEQ_DEBUG | L.AICP_RUN_TIME_NN | 3)
    q = L.default_localization_params(merge=False, debug=True)
    assert q.flags == L.AICP_SEQ_DEBUG


def test_null_arguments_are_invalid_without_a_device(L):
    done = C.c_size_t(7)
    assert L.lib.aicp_hip_map_sequence_run(None, None, None, None, None, None, None, 0, None, None,
                                           C.byref(done)) == L.AICP_ERR_INVALID
    t = L.LocalizationTiming()
    assert L.lib.aicp_hip_last_localization_timing(None, C.byref(t)) == L.AICP_ERR_INVALID
