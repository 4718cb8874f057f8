"""The mapping session's built map on the device (AppSession(keep_aligned_map=True): aligned_map,
take_aligned_map), the go-back (MapSession.start_go_back) and the start on a loaded map
(AppSession.start_on_map), bit for bit against the host loops of tests/mapping_reference.py: the
map as the concatenation of reference() downloads, App on the prior map from a given count and
initialT_ over one-reading calls, and the crop at the pose as a plain session's first cloud.

Streams are synthetic pre-filtered clouds of about 3000 points, cut so that promoted readings have
3072 and 3073 points among others; every run is computed once per module and shared."""
import functools

import numpy as np
import pytest

import mapping_reference as mr
import session_reference as sr
import svm_reference as sv
from aicp_mapping_amd import synthetic as sy
from mapping_reference import same_bits, strip
from test_session import fill, scene_sweeps

pytestmark = pytest.mark.gpu
RES = float(np.float32(0.2))
F32 = np.float32
SIZES = [3073, 3072, 3073, 3073, 3072, 3000, 3073, 2817, 3073, 3073]  # reading i's points
N_MAP, N_LOC = 6, 6  # readings of the mapping run before the go-back, localisation readings after it
CROP = 12.0


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def stream(jump_at=None):
    """12 pre-filtered readings along x; reading i < 10 cut to SIZES[i] points."""
    jumps = {jump_at: (0.0, -0.8, 0.0)} if jump_at is not None else None
    st = sy.make_stream(n_readings=N_MAP + N_LOC, n_points=3073, seed=7, half=18.0, jumps=jumps)
    st.readings = [np.ascontiguousarray(r[:SIZES[i]]) if i < len(SIZES) else r for i, r in enumerate(st.readings)]
    return st


def params(L, debug, freq, max_corr=1.0):
    return L.default_sequence_params(reference_update_frequency=freq, max_correction_magnitude=max_corr, resolution=RES,
                                     flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0))


def plain(ctx, L, st, debug, freq, keep, n=10, max_corr=1.0, cfg=None, prefilter=None):
    """The first n readings of st through a plain session; the session is closed."""
    from aicp_mapping_amd.session import AppSession

    s = AppSession(ctx, cfg=cfg, params=params(L, debug, freq, max_corr), prefilter=prefilter, keep_aligned_map=keep)
    steps = [functools.partial(s.process, st.readings[i], st.origins[i], raise_on_error=False) for i in range(n)]
    run = mr.drive(s, lambda: s.start(st.first, st.first_origin), steps, keep)
    s.close()
    return run


_RUNS = {}


def both(ctx, L, key, make):
    """(keeping on, keeping off) of one configuration, computed once."""
    if key not in _RUNS:
        _RUNS[key] = (make(True), make(False))
    return _RUNS[key]


def pose_at(origin):
    P = np.eye(4)
    P[:3, 3] = origin
    return P


# ---- 1. the map equals the reference loop -----------------------------------------------------------
@pytest.mark.parametrize("debug,freq", [(False, 2), (True, 5), (True, 2)], ids=["robot-2", "debug-5", "debug-2"])
def test_map_equals_reference_loop_and_outputs_are_unchanged(ctx, L, debug, freq):
    on, off = both(ctx, L, ("plain", debug, freq), lambda keep: plain(ctx, L, stream(), debug, freq, keep))
    assert all(o["status"] == 0 and o["accepted"] for o in on["out"])
    promoted = [i for i, o in enumerate(on["out"]) if o["is_reference"]]
    assert promoted == list(range(freq - 1, 10, freq))
    assert {3072, 3073} <= {SIZES[i] for i in promoted}
    mr.same_maps(on, off)  # after the start and after every call, byte for byte
    mr.same_outputs(on, off)  # T, results, kept, state and reference: keeping changes none of them
    assert same_bits(on["map0"], stream().first)  # (pre-filtered entry: the first cloud as given)
    sizes = [len(m) for m in on["maps"]]
    assert sizes == list(np.cumsum([SIZES[i] if i in promoted else 0 for i in range(10)]) + len(stream().first))


def test_map_growth_reallocates_and_still_matches(ctx, L):
    """The map is created exactly as large as the first cloud, so the stream's appends outgrow it
    more than once: at least two reallocations, and the content is the reference loop's."""
    on, off = both(ctx, L, ("plain", False, 2), lambda keep: plain(ctx, L, stream(), False, 2, keep))
    caps = [len(stream().first)] + on["caps"]
    assert sum(a != b for a, b in zip(caps, caps[1:])) >= 2, caps
    assert all(c >= len(m) for c, m in zip(on["caps"], on["maps"]))
    mr.same_maps(on, off)


def test_keeping_off_is_the_session_as_it_was(ctx, oracle, L):
    """With keeping off the stream's results are the host loop's of tests/session_reference.py."""
    st = stream()
    _, off = both(ctx, L, ("plain", False, 2), lambda keep: plain(ctx, L, st, False, 2, keep))
    loop, _ = sr.replay(sr.CtxBackend(ctx, L, resolution=RES), oracle, st.first, st.first_origin, st.readings[:10],
                        st.origins[:10], freq=2, debug=False, raw=False)
    for i, rec in enumerate(loop):
        assert same_bits(off["T"][i], rec["T"]), i
        assert off["out"][i]["icp"] == rec["icp"], i
        assert (off["out"][i]["accepted"], off["out"][i]["is_reference"], off["out"][i]["reference"]) == \
            (rec["accepted"], rec["is_reference"], rec["reference"]), i


@functools.lru_cache(maxsize=None)
def raw_stream():
    """Raw readings; reading 3 carries a 0.8 m jump (dropped at max_correction_magnitude 0.4)."""
    return sy.make_stream(n_readings=8, n_points=20000, seed=8, half=12.0, jumps={3: (0, -0.8, 0)})


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_raw_input_and_a_dropped_reading_at_the_promotion_turn(ctx, L, debug):
    """Raw readings through the session's pre-filter, frequency 4. Reading 3 is dropped when the
    count says it would be promoted (room was made for it): the map's size stays, and reading 4 is
    promoted in its place."""
    on, off = both(ctx, L, ("raw", debug), lambda keep: plain(ctx, L, raw_stream(), debug, 4, keep, n=8, max_corr=0.4,
                                                               prefilter=True))
    assert [o["accepted"] for o in on["out"]] == [1, 1, 1, 0, 1, 1, 1, 1]
    assert [o["is_reference"] for o in on["out"]] == [0, 0, 0, 0, 1, 0, 0, 0]
    mr.same_maps(on, off)
    mr.same_outputs(on, off)
    assert len(on["maps"][3]) == len(on["maps"][2]) and len(on["maps"][4]) == len(on["maps"][3]) + on["kept"][4]
    assert len(on["map0"]) < 20000  # the first cloud as pre-filtered, not as given


def test_a_reading_that_ends_the_session_appends_nothing(ctx, L):
    """Reading 1, at the promotion turn of frequency 2, lies 200 m away with a 5 m matcher radius."""
    from aicp_mapping_amd.session import AppSession

    st = stream()
    far = (st.readings[1] + F32(200.0)).astype(F32)
    s = AppSession(ctx, cfg=L.default_config(nn_max_dist=5.0), params=params(L, False, 2), keep_aligned_map=True)
    s.start(st.first, st.first_origin)
    T, res, kept = s.process(st.readings[0], st.origins[0])
    assert res["accepted"] and not res["is_reference"]
    T, res, kept = s.process(far, st.origins[1] + 200.0, raise_on_error=False)
    assert res["rc"] == L.AICP_ERR_CONVERGENCE and s.state()["ended"]
    m = s.aligned_map
    assert len(m) == len(st.first) and same_bits(m.getCloud(), st.first)
    assert m.capacity >= len(st.first) + len(far)  # (room had been made)
    s.close()


def test_readings_from_the_accumulator(ctx, L):
    """start(acc) and process(acc): the map is the reference loop's of a twin fed the downloads."""
    from aicp_mapping_amd.accumulator import SweepAccumulator
    from aicp_mapping_amd.session import AppSession

    cap = max(sum(len(s) for s in scene_sweeps(k)[0]) for k in range(4))
    acc = SweepAccumulator(ctx, cap, batch_size=3)
    a = AppSession(ctx, params=params(L, False, 1), prefilter=True, keep_aligned_map=True)
    b = AppSession(ctx, params=params(L, False, 1), prefilter=True)
    o0 = fill(acc, 0)
    a.start(acc, o0)
    b.start(acc.getCloud(), o0)
    host = b.reference()[0]
    assert same_bits(a.aligned_map.getCloud(), host)
    for k in (1, 2, 3):
        acc.clear()
        o = fill(acc, k)
        Ta, ra, ka = a.process(acc, o)
        Tb, rb, kb = b.process(acc.getCloud(), o)
        assert same_bits(Ta, Tb) and ra == rb and ka == kb and ra["is_reference"], k
        host = np.concatenate([host, b.reference()[0]], 0)
        assert same_bits(a.aligned_map.getCloud(), host), k
    for s in (a, b):
        s.close()
    acc.free()


def test_point_to_point_chain(ctx, L):
    cfg = L.default_config(point_to_point=True)
    on, off = both(ctx, L, "p2p", lambda keep: plain(ctx, L, stream(), True, 1, keep, n=4, cfg=cfg))
    assert all(o["is_reference"] and o["icp"]["iterations"] > 0 for o in on["out"])
    mr.same_maps(on, off)
    mr.same_outputs(on, off)


# ---- a risk session: gated readings are appended unmoved, registered ones moved ---------------------
def test_risk_session_gated_and_registered_promotions(ctx, L, tmp_path):
    import risk_reference as rr
    from aicp_mapping_amd.session import AppSession

    st = raw_stream()
    first_pose = rr.pose(0.0, st.first_origin)
    poses = [rr.pose(4.0 * (i + 1), st.origins[i]) for i in range(8)]

    def run(X, keep):
        model = L.SvmModel(sv.write_threshold_model(str(tmp_path / f"thr_{X:.6f}.xml"), X))
        s = AppSession(ctx, params=params(L, False, 2), prefilter=True, keep_aligned_map=keep,
                       risk=dict(model=model, threshold=0.5, params=L.default_risk_params(angular_view=270.0)))
        steps = [functools.partial(s.process, st.readings[i], pose=poses[i], raise_on_error=False) for i in range(8)]
        out = mr.drive(s, lambda: s.start(st.first, pose=first_pose), steps, keep)
        s.close()
        model.close()
        return out

    free = run(0.0, False)  # nothing gates: the overlaps, to place the gate between them
    ovs = sorted(e[0]["octree_overlap"] for e in free["extra"])
    gaps = np.diff(ovs)
    k = int(np.argmax(gaps))  # the widest gap between two readings' overlaps
    assert all(e[0]["registered"] for e in free["extra"]) and gaps[k] >= 2.0, ovs
    X = 0.5 * (ovs[k] + ovs[k + 1])
    on, off = run(X, True), run(X, False)
    registered = [e[0]["registered"] for e in on["extra"]]
    promoted = [o["is_reference"] for o in on["out"]]
    assert 0 in registered and any(r and p for r, p in zip(registered, promoted)), (registered, promoted)
    assert all(p for r, p in zip(registered, promoted) if not r)  # a gated reading is the reference at once
    mr.same_maps(on, off)
    mr.same_outputs(on, off)
    g = registered.index(0)  # the gated reading's bytes, unmoved, are the map's tail after its call
    assert same_bits(on["maps"][g][-on["kept"][g]:], on["refs"][g][0])


# ---- restart, take --------------------------------------------------------------------------------------
def test_restart_replaces_the_map_and_take_hands_it_over(ctx, L):
    from aicp_mapping_amd.session import AppSession

    st = stream()
    s = AppSession(ctx, params=params(L, False, 1))
    s.start(st.first, st.first_origin)
    with pytest.raises(L.AicpError) as e:  # keeping is off
        s.aligned_map
    assert e.value.code == L.AICP_ERR_INVALID
    s.keep_aligned_map(True)
    with pytest.raises(L.AicpError):  # on, but this start made none
        s.aligned_map
    s.start(st.first, st.first_origin)
    s.process(st.readings[0], st.origins[0])
    assert len(s.aligned_map) == len(st.first) + SIZES[0]
    with pytest.raises(L.AicpError):  # a start that fails leaves the old map as it was
        s.start(np.zeros((0, 3), F32))
    assert len(s.aligned_map) == len(st.first) + SIZES[0]
    s.start(st.readings[2], st.origins[2])  # a start that succeeds replaces it
    assert same_bits(s.aligned_map.getCloud(), st.readings[2])
    s.process(st.readings[3], st.origins[3])
    want = np.concatenate([st.readings[2], s.reference()[0]], 0)
    taken = s.take_aligned_map()
    assert same_bits(taken.getCloud(), want)
    with pytest.raises(L.AicpError) as e:
        s.aligned_map
    assert e.value.code == L.AICP_ERR_INVALID
    with pytest.raises(L.AicpError):
        s.take_aligned_map()
    T, res, kept = s.process(st.readings[4], st.origins[4])  # the session keeps running, the taken map stays
    assert res["is_reference"] and len(taken) == len(want) and same_bits(taken.getCloud(), want)
    s.start(st.first, st.first_origin)  # the next start keeps a map again
    assert len(s.aligned_map) == len(st.first)
    s.close()
    assert same_bits(taken.getCloud(), want)  # the caller's, past the session
    taken.free()


# ---- the go-back ----------------------------------------------------------------------------------------
LOC = dict(reference_update_frequency=3, map_refilter_every=4, max_correction_magnitude=0.4, crop_min=-CROP,
           crop_max=CROP)


def mapping_run(ctx, L, st, freq=2):
    """The first N_MAP readings through a keeping session, left open: (session, accepted readings)."""
    from aicp_mapping_amd.session import AppSession

    s = AppSession(ctx, params=params(L, False, freq), keep_aligned_map=True)
    s.start(st.first, st.first_origin)
    acc = 0
    for i in range(N_MAP):
        acc += s.process(st.readings[i], st.origins[i])[1]["accepted"]
    return s, acc


def localise(ctx, L, ms, st, keys=("status", "accepted", "merged", "refiltered", "map_points", "crop_points")):
    out = []
    for i in range(N_MAP, N_MAP + N_LOC):
        T, d, kept = ms.process(st.readings[i], pose_at(st.origins[i]))
        out.append(dict(T=T, icp=d["icp"], corrected_origin=d["corrected_origin"], **{k: d[k] for k in keys}))
    return out


@pytest.mark.parametrize("jump", [None, N_MAP], ids=["steady", "jump-on-first"])
def test_go_back_equals_the_host_loop(ctx, L, jump):
    from aicp_mapping_amd.map_session import MapSession

    st = stream(jump)
    s, acc = mapping_run(ctx, L, st)
    assert acc == N_MAP
    initT = s.state()["initial_T"]
    prior = s.take_aligned_map()
    map_pts = prior.getCloud()
    ms = MapSession(ctx, prior, params=L.default_localization_params(**LOC))
    ms.start_go_back(s)
    s.close()  # neither handle needs the other
    state = ms.state()
    assert state["count"] == 1 + N_MAP and state["n_processed"] == 0 and not state["ended"]
    assert same_bits(state["initial_T"], initT) and not np.array_equal(initT, np.eye(4, dtype=F32))
    got = localise(ctx, L, ms, st)
    poses = [pose_at(o) for o in st.origins[N_MAP:]]
    want, final, n_clouds, initT_end = mr.go_back_loop(ctx, L, map_pts, st.readings[N_MAP:], poses, 1 + N_MAP, initT, 3, 4,
                                                       0.4, CROP)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g["T"], w["T"]), i
        for k in ("status", "accepted", "merged", "refiltered", "map_points", "crop_points", "icp"):
            assert g[k] == w[k], (i, k, g[k], w[k])
        assert same_bits(g["corrected_origin"], w["corrected_origin"], np.float64), i
    assert same_bits(prior.getCloud(), final)
    state = ms.state()
    assert state["count"] == n_clouds and same_bits(state["initial_T"], initT_end)
    accepted = [g["accepted"] for g in got]
    if jump is None:
        # count 7 at the go-back: merges where (n_clouds - 1) % 3 == 0, not where a count of 0 puts them
        assert accepted == [1] * N_LOC
        assert [i for i, g in enumerate(got) if g["merged"]] == [2, 5]
        assert [i for i, g in enumerate(got) if g["refiltered"]] == [1, 5]
    else:
        # the drop test is live on the first localisation reading; a plain start on the same map
        # (count 0: the first cloud of the graph is never dropped) accepts it
        assert accepted[0] == 0 and got[0]["status"] == 0 and 1 in accepted
        from aicp_mapping_amd.prior_map import PriorMap

        m2 = PriorMap(ctx, map_pts)
        fresh = MapSession(ctx, m2, params=L.default_localization_params(**LOC))
        fresh.start()
        T, d, kept = fresh.process(st.readings[N_MAP], pose_at(st.origins[N_MAP]))
        assert d["accepted"] == 1 and same_bits(T, got[0]["T"])
        fresh.close()
        m2.free()
    ms.close()
    prior.free()


def test_go_back_refusals_leave_the_state(ctx, L):
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.prior_map import PriorMap
    from aicp_mapping_amd.session import AppSession

    st = stream()
    m = PriorMap(ctx, st.first)
    ms = MapSession(ctx, m, params=L.default_localization_params(**LOC))
    ms.start()
    ms.process(st.readings[0], pose_at(st.origins[0]))
    before = ms.state()

    def refused(target, src, context=ctx):
        with pytest.raises(L.AicpError) as e:
            context.check(L.lib.aicp_hip_mapsession_start_go_back(context.h, target.h, target.map.h, src.h))
        assert e.value.code == L.AICP_ERR_INVALID
        after = ms.state()
        assert after.pop("initial_T").tobytes() == before["initial_T"].tobytes()
        assert after == {k: v for k, v in before.items() if k != "initial_T"}

    s = AppSession(ctx, cfg=L.default_config(nn_max_dist=5.0), params=params(L, False, 2))
    refused(ms, s)  # not started
    s.start(st.first, st.first_origin)
    bm = BuiltMap(ctx, st.first)
    built = MapSession(ctx, bm, params=L.default_built_map_params())
    refused(built, s)  # the built-map policy
    other = L.Context(0)
    refused(ms, s, other)  # from lives on another context
    other.close()
    s.process((st.readings[0] + F32(200.0)).astype(F32), st.origins[0] + 200.0, raise_on_error=False)
    assert s.state()["ended"]
    refused(ms, s)  # ended: App's worker is dead
    s.start(st.first, st.first_origin)  # revived: accepted now, at count 1 (the first cloud alone)
    ms.start_go_back(s)
    assert ms.state()["count"] == 1 and ms.state()["n_processed"] == 0
    for x in (built, ms, s):
        x.close()
    bm.free()
    m.free()


# ---- the start on a loaded map --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loaded_map():
    return np.ascontiguousarray(sy.make_stream(n_readings=1, n_points=6000, seed=7, half=18.0).first)


@pytest.mark.parametrize("debug", [False, True], ids=["robot", "debug"])
def test_start_on_map_equals_the_reference_loop(ctx, L, debug):
    """Frequency 5, 8 readings: the first is promoted whatever the frequency. Robot mode: it carries
    a jump beyond max_correction_magnitude and is accepted (no drop test on an empty graph). Debug
    mode: the later readings are moved by the carried initialT_ (a jump on the first reading alone
    would have every later one dropped, so that stream has none)."""
    from aicp_mapping_amd.prior_map import PriorMap
    from aicp_mapping_amd.session import AppSession

    st = stream(None if debug else 0)
    pose = pose_at(st.origins[0])
    m = PriorMap(ctx, loaded_map())
    s = AppSession(ctx, params=params(L, debug, 5, 0.4), keep_aligned_map=True)
    steps = [functools.partial(s.process, st.readings[i], st.origins[i], raise_on_error=False) for i in range(8)]
    run = mr.drive(s, lambda: s.start_on_map(m, pose, crop=CROP), steps, True, on_map=True)
    crop = m.crop(-CROP, CROP, pose.astype(F32))
    m.free()  # not needed after the start
    assert len(run["map0"]) == 0  # no first cloud
    want, maps = mr.on_map_loop(ctx, L, loaded_map(), pose, CROP, st.readings[:8], st.origins[:8], 5, 0.4, debug,
                                resolution=RES)
    assert 0 < len(crop) < len(loaded_map())
    first = run["out"][0]
    assert first["accepted"] and first["is_reference"] and first["reference"] == -1
    if not debug:
        assert max(abs(run["T"][0][:3, 3])) > 0.4  # beyond the limit, and accepted
    else:
        assert not np.array_equal(run["states"][1]["initial_T"], np.eye(4, dtype=F32))
    assert [o["is_reference"] for o in run["out"]] == [1, 0, 0, 0, 0, 1, 0, 0]
    for i, w in enumerate(want):
        assert same_bits(run["T"][i], w["T"]), i
        assert run["out"][i] == w["out"], (i, run["out"][i], w["out"])
        assert run["kept"][i] == w["kept"], i
        assert same_bits(run["states"][i]["initial_T"], w["initial_T"]), i  # the host's float product
        assert same_bits(run["refs"][i][0], w["ref"][0]) and np.array_equal(run["refs"][i][1], w["ref"][1]), i
        assert same_bits(run["maps"][i], maps[i]), i
    # with keeping on, the map's first points are the first reading's promoted reference
    assert same_bits(run["maps"][-1][:SIZES[0]], run["refs"][0][0])
    assert run["states"][-1]["n_processed"] == 8 and not run["states"][-1]["ended"]
    s.close()


def test_start_on_map_refusals(ctx, L, tmp_path):
    from aicp_mapping_amd.prior_map import PriorMap
    from aicp_mapping_amd.session import AppSession

    st = stream()
    m = PriorMap(ctx, loaded_map())
    s = AppSession(ctx, params=params(L, False, 5))
    s.start(st.first, st.first_origin)
    s.process(st.readings[0], st.origins[0])
    before, ref = s.state(), s.reference()[0]
    with pytest.raises(L.AicpError) as e:  # an empty crop: 500 m away
        s.start_on_map(m, pose_at([500.0, 0.0, 0.0]), crop=CROP)
    assert e.value.code == L.AICP_ERR_INVALID
    after = s.state()
    assert after["n_processed"] == 1 and not after["ended"] and same_bits(s.reference()[0], ref)
    assert same_bits(after["initial_T"], before["initial_T"])
    T, res, kept = s.process(st.readings[1], st.origins[1])  # a running session keeps running
    assert res["status"] == 0 and res["accepted"]
    s.close()
    model = L.SvmModel(sv.write_threshold_model(str(tmp_path / "thr.xml"), 0.0))
    r = AppSession(ctx, params=params(L, False, 5), risk=dict(model=model, threshold=0.5))
    with pytest.raises(L.AicpError) as e:  # plain sessions only
        r.start_on_map(m, pose_at(st.origins[0]), crop=CROP)
    assert e.value.code == L.AICP_ERR_INVALID
    with pytest.raises(L.AicpError):  # nothing changed: it has not started
        r.state()
    r.close()
    model.close()
    m.free()


def test_load_map_from_file_feeds_the_start(ctx, L, tmp_path):
    """A PLY file written here -> load_map_from_file -> start_on_map: the node's path."""
    from aicp_mapping_amd.prior_map import load_map_from_file
    from aicp_mapping_amd.session import AppSession

    pts = loaded_map()
    path = str(tmp_path / "map.ply")
    with open(path, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(pts)}\nproperty float x\n"
                "property float y\nproperty float z\nend_header\n".encode("ascii"))
        f.write(pts.astype("<f4").tobytes())
    m = load_map_from_file(ctx, path)
    assert same_bits(m.getCloud(), ctx.prefilter(pts)) and 0 < len(m) < len(pts)
    st = stream()
    s = AppSession(ctx, params=params(L, False, 5))
    s.start_on_map(m, pose_at(st.origins[0]), crop=CROP)
    T, res, kept = s.process(st.readings[0], st.origins[0])
    assert res["status"] == 0 and res["accepted"] and res["is_reference"]
    s.close()
    m.free()
