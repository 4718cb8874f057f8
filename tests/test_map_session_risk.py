"""The live map sessions with failure_prediction_mode (aicp_hip_mapsession_create_risk and the _risk
calls, MapSession(..., risk=...)): the alignment-risk gate served one reading per call on the prior
map and on the built map, the gated branch taken on the device by k_session_map_gate.

The bar is exact: reading by reading the session gives the bits of the host loop of
tests/map_session_risk_reference.py, which composes the same rules from public one-reading calls
(T, every result field, the record's fov_overlap, octree_overlap, alignability and trimmed_ratio,
count and initialT_ after every call, the final map). The record's raw and risk are the bits of
aicp_hip_svm_predict on the loop's sample, and lie within tests/test_svm.py's bar of the loop's numpy
classifier (numpy's pow and exp are not the device's; the decisions are kept away from the
threshold). Where the gate falls is decided on the host loop alone, before the session is looked at.
Fixtures: tests/raw_stream_reference.py's small worlds; runs are computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest

import map_session_risk_reference as mr
import raw_stream_reference as rs
import risk_reference as rr
import svm_reference as sr
from aicp_mapping_amd import synthetic as sy
from test_alignment_risk import ORIGIN_A, ORIGIN_B, scene_cloud
from test_raw_stream import APPEND, make_map, params
from test_session import scene_sweeps
from test_session_risk import edge_reading

pytestmark = pytest.mark.gpu

STREAMS = ["prior", "built"]
MODES = [False, True]
MODE_IDS = ["robot", "debug"]
F32 = np.float32
VIEW = 270.0
# how far every reading's feature stays from the gate's X: the session and the loop classify the same
# bits, and the classifier's own rounding (a float product, a float sum: svm_reference.raw_bar) is a
# few ulps of X, so any margin far above 1e-6 of X keeps the decision out of reach of it. The overlap
# is in percent (the margin of tests/test_session_risk.py); alignabilities of these worlds are of
# the order 1e-2, whose float ulp is 1e-9: 1e-4 is five decades above the rounding
MARGIN = dict(built=0.5, prior=1e-4)


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(oracle):
    """stream -> (map, raw readings, poses, origins); read only."""
    return dict(prior=rs.prior_world(oracle), built=rs.built_world(oracle))


@pytest.fixture(scope="module")
def models(L, tmp_path_factory):
    """"golden", or (stream, X) -> (SvmModel, numpy model). Built map: raw = overlap - X
    (svm_reference.write_threshold_model); prior map, where the overlap is the constant 50:
    raw = alignability - X (support vector (0, 1)). risk > 0.5 <=> the feature < X."""
    d = tmp_path_factory.mktemp("svm")
    made = {}

    def get(key):
        if key not in made:
            if key == "golden":
                path = sr.golden(sr.MODELS["opencv3"][0])
            elif key[0] == "built":
                path = sr.write_threshold_model(str(d / f"ov_{key[1]:.9f}.xml"), key[1])
            else:
                path = sr.write_model(str(d / f"al_{key[1]:.9f}.xml"), [[0.0, 1.0]], [1.0], key[1], 1.0, 1.0, 0.0)
            made[key] = (L.SvmModel(path), sr.read_model(path))
        return made[key]

    yield get
    for m, _ in made.values():
        m.close()


def risk_params(L):
    return L.default_risk_params(angular_view=VIEW)


def same_bits(a, b, dtype=F32):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def f32(x):
    return float(F32(x))


def session(ctx, L, stream, m, model, thr, debug=False, raw=True, cfg=None, monitor=None, **kw):
    from aicp_mapping_amd.map_session import MapSession

    return MapSession(ctx, m, cfg=cfg, params=params(L, stream, debug, **kw), prefilter=True if raw else None,
                      risk=dict(model=model, threshold=thr, params=risk_params(L)), monitor=monitor)


def feed(ctx, L, stream, mp, reads, poses, model, thr, debug=False, raw=True, cfg=None, between=None, monitor=None,
         maps=False, **kw):
    """The readings one by one through a risk session on a fresh map."""
    m = make_map(ctx, stream, mp)
    s = session(ctx, L, stream, m, model, thr, debug, raw, cfg, monitor, **kw)
    s.start()
    out = dict(T=[], res=[], kept=[], rec=[], states=[], sizes=[], maps=[], mon=[], rc=0)
    for i, (r, P) in enumerate(zip(reads, poses)):
        T, d, k, rec = s.process(r, P, raise_on_error=False)
        out["rc"] = d.pop("rc")
        out["T"].append(T)
        out["res"].append(d)
        out["kept"].append(k)
        out["rec"].append(rec)
        out["states"].append(s.state())
        out["sizes"].append(len(m))
        if maps:
            out["maps"].append(m.getCloud())
        if monitor:
            out["mon"].append(s.last_monitor())
        if out["rc"]:
            break
        if between:
            between(i, m)
    out["final"] = m.getCloud()
    out["error"] = ctx.last_error()
    s.close()
    m.free()
    return out


def loop(ctx, L, stream, world, ref_model, thr, debug, n=None, cfg=None, prefilter=True, **kw):
    mp, raws, poses, _ = world
    n = n or len(raws)
    p = params(L, stream, debug, **kw)
    built = stream == "built"
    prm = dict(crop_min=p.crop_min, crop_max=p.crop_max, resolution=p.resolution if built else 0.0)
    blocks = mr.CtxBlocks(ctx, L, ref_model, built, prm, risk_params(L), cfg=cfg, prefilter=prefilter)
    return mr.host_loop(blocks, mp, raws[:n], poses[:n], p.reference_update_frequency, p.max_correction_magnitude,
                        thr, debug, refilter_every=0 if built else p.map_refilter_every,
                        merge=True if built else bool(p.flags & L.AICP_LOC_MERGE))


def feature(stream, c):
    return c["overlap"] if stream == "built" else c["alignability"]


def expected_icp(stream, c):
    """The reading's aicp_icp_stats as the header states them, from the loop's calls."""
    built = stream == "built"
    if c["registered"]:
        st = dict(c["stats"])
        if built:
            st.update(overlap_percent=f32(c["overlap"]), overlap_keys=list(c["keys"]))
        return st
    return dict(status=0, iterations=0, converged=0, degenerate_normals=0, inlier_ratio=0.0,
                trimmed_ratio=f32(c["ratio"]), overlap_percent=f32(c["overlap"]), tree_depth=0, nn_points_touched=0,
                nn_nodes_touched=0, overlap_keys=list(c["keys"]) if built else [0, 0, 0])


def equals_loop(ctx, stream, run, comp, model, ref_model):
    """Reading by reading, and the final map."""
    assert run["rc"] == 0 and len(run["res"]) == len(comp)
    for i, c in enumerate(comp):
        d, rec, st = run["res"][i], run["rec"][i], run["states"][i]
        assert c["status"] == 0 and d["status"] == 0, i
        got = (rec["registered"], d["accepted"], d[APPEND[stream]], d.get("refiltered", 0))
        assert got == (c["registered"], c["accepted"], c["append"], c["refilter"]), (i, got)
        assert (run["kept"][i], rec["n_read"], d["map_points"], d["crop_points"]) == \
            (c["kept"], c["kept"], c["map_points"], c["crop_points"]), i
        assert same_bits(run["T"][i], c["T"]), i
        want_origin = [0.0, 0.0, 0.0] if c["corrected_origin"] is None else c["corrected_origin"]
        assert same_bits(d["corrected_origin"], want_origin, np.float64), i
        assert d["icp"] == expected_icp(stream, c), (i, d["icp"], expected_icp(stream, c))
        for k, v in (("fov_overlap", c["fov_overlap"]), ("octree_overlap", c["overlap"]),
                     ("alignability", c["alignability"]), ("trimmed_ratio", c["ratio"])):
            assert F32(rec[k]).tobytes() == F32(v).tobytes(), (i, k, rec[k], v)
        X = np.array([[c["overlap"], c["alignability"]]], F32)
        raw_d, risk_d = ctx.svm_predict(model, X)
        assert F32(rec["raw"]).tobytes() == raw_d.tobytes() and np.float64(rec["risk"]).tobytes() == risk_d.tobytes(), i
        raw_n, risk_n, terms = sr.predict(ref_model, X)
        bar = sr.raw_bar(raw_n, terms)[0]
        assert abs(rec["raw"] - raw_n[0]) <= bar and abs(rec["risk"] - risk_n[0]) <= 0.25 * bar + 1e-15, i
        assert (st["count"], st["n_processed"], st["ended"]) == (c["count"], i + 1, False), i
        assert same_bits(st["initial_T"], c["initial_T"]), i
        assert run["sizes"][i] == len(c["map"]), i
    assert same_bits(run["final"], comp[-1]["map"])


def place_gate(stream, free):
    """X in the widest gap between the ungated loop's features."""
    v = sorted(feature(stream, c) for c in free)
    gaps = [(b - a, 0.5 * (a + b)) for a, b in zip(v, v[1:])]
    gap, X = max(gaps)
    assert gap >= 2.0 * MARGIN[stream], (v, gap)
    return float(X)


# ---- case 1: a gate in mid-window ---------------------------------------------------------------------
_MID = {}
# built map: at the fixture's frequency 3 the reading that jumps (3) comes right behind a reference;
# at 5 the gate falls with three readings counted, and reading 8 is still a reference by the count
MID_KW = dict(prior={}, built=dict(reference_update_frequency=5))


def mid_window(ctx, L, worlds, models, stream, debug, **kw):
    """X from the ungated host loop, the gated host loop with its assertions, and the session's run
    (computed once per policy, mode and parameters)."""
    kw = dict(MID_KW[stream], **kw)
    key = (stream, debug, tuple(sorted(kw.items())))
    if key not in _MID:
        golden = models("golden")[1]
        free = loop(ctx, L, stream, worlds[stream], golden, 1.0, debug, **kw)
        assert all(c["registered"] and c["status"] == 0 for c in free)
        X = place_gate(stream, free)
        model, ref_model = models((stream, X))
        comp = loop(ctx, L, stream, worlds[stream], ref_model, 0.5, debug, **kw)
        print(stream, "debug" if debug else "robot", kw, "features", [round(float(feature(stream, c)), 4) for c in comp],
              "X", X, "registered", [c["registered"] for c in comp], "accepted", [c["accepted"] for c in comp],
              "append", [c["append"] for c in comp], "count", [c["count"] for c in comp])
        assert all(abs(feature(stream, c) - X) >= MARGIN[stream] for c in comp)
        reg = [c["registered"] for c in comp]
        assert 0 in reg and 1 in reg
        mp, raws, poses, _ = worlds[stream]
        _MID[key] = dict(X=X, comp=comp, model=model, ref_model=ref_model, kw=kw,
                         run=feed(ctx, L, stream, mp, raws, poses, model, 0.5, debug, **kw))
    return _MID[key]


@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_gate_in_mid_window(ctx, L, worlds, models, stream, debug):
    m = mid_window(ctx, L, worlds, models, stream, debug)
    comp, run = m["comp"], m["run"]
    # in mid-window: a gated reading that is not the first, with the count under way, and a
    # registered reading behind it
    gated = [i for i, c in enumerate(comp) if not c["registered"]]
    assert any(i > 0 and comp[i - 1]["count"] != 0 for i in gated)
    assert any(c["registered"] for c in comp[gated[0] + 1:])
    equals_loop(ctx, stream, run, comp, m["model"], m["ref_model"])
    for i in gated:
        assert np.array_equal(run["T"][i], np.eye(4, dtype=F32)) and run["res"][i]["icp"]["iterations"] == 0
        if i:
            assert same_bits(run["states"][i]["initial_T"], run["states"][i - 1]["initial_T"])
        if stream == "built":
            assert run["states"][i]["count"] == 0 and run["sizes"][i] == run["res"][i]["map_points"] + run["kept"][i]
        else:
            assert run["res"][i]["merged"] == 0


# ---- case 2: nothing gates --------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_threshold_one_is_the_plain_session(ctx, L, worlds, models, stream, debug):
    """The golden model under threshold 1.0: a plain MapSession on a twin map, bit for bit."""
    from aicp_mapping_amd.map_session import MapSession

    mp, raws, poses, _ = worlds[stream]
    run = feed(ctx, L, stream, mp, raws, poses, models("golden")[0], 1.0, debug)
    assert run["rc"] == 0 and all(r["registered"] == 1 for r in run["rec"])
    m = make_map(ctx, stream, mp)
    p = MapSession(ctx, m, params=params(L, stream, debug), prefilter=True)
    p.start()
    for i, (r, P) in enumerate(zip(raws, poses)):
        T, d, kept = p.process(r, P)
        d.pop("rc")
        assert same_bits(run["T"][i], T), i
        assert run["res"][i] == d, (i, run["res"][i], d)
        assert run["kept"][i] == kept and run["sizes"][i] == len(m), i
        st = p.state()
        assert run["states"][i]["count"] == st["count"] and same_bits(run["states"][i]["initial_T"], st["initial_T"]), i
    assert same_bits(run["final"], m.getCloud())
    p.close()
    m.free()


# ---- case 2b: the pre-filtered entry ---------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, 1.0], ids=["all_gated", "none_gated"])
@pytest.mark.parametrize("debug", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("stream", STREAMS)
def test_prefiltered_readings(ctx, L, oracle, models, stream, debug, thr):
    """pf_read NULL: the readings come pre-filtered (debug mode moves the filtered cloud). The golden
    model's risk lies strictly inside (0, 1), so thresholds 0.0 and 1.0 decide without a margin."""
    import built_map_reference as bm
    import localization_reference as lr

    n = 6
    world = ((lr.make_map(oracle),) + lr.make_stream(n, lr.JUMPS)) if stream == "prior" else \
        ((bm.make_first_cloud(oracle),) + bm.make_stream())
    model, ref_model = models("golden")
    comp = loop(ctx, L, stream, world, ref_model, thr, debug, n=n, prefilter=False)
    assert [c["registered"] for c in comp] == [int(thr == 1.0)] * n and all(0.0 < c["risk"] < 1.0 for c in comp)
    run = feed(ctx, L, stream, world[0], world[1][:n], world[2][:n], model, thr, debug, raw=False)
    assert run["kept"] == [len(r) for r in world[1][:n]]
    equals_loop(ctx, stream, run, comp, model, ref_model)


# ---- case 3: everything gates -----------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_threshold_zero_gates_every_reading(ctx, L, worlds, models, stream):
    mp, raws, poses, _ = worlds[stream]
    n = 6
    run = feed(ctx, L, stream, mp, raws[:n], poses[:n], models("golden")[0], 0.0, False, maps=True)
    assert run["rc"] == 0
    assert [r["registered"] for r in run["rec"]] == [0] * n and all(0.0 < r["risk"] < 1.0 for r in run["rec"])
    assert all(np.array_equal(T, np.eye(4, dtype=F32)) for T in run["T"])
    assert all(np.array_equal(s["initial_T"], np.eye(4, dtype=F32)) for s in run["states"])
    assert [(d["status"], d["accepted"], d["icp"]["iterations"]) for d in run["res"]] == [(0, 1, 0)] * n
    before = np.ascontiguousarray(mp, F32)
    every = params(L, stream).map_refilter_every if stream == "prior" else 0
    for i in range(n):
        d = run["res"][i]
        assert d["corrected_origin"] == [float(x) for x in np.asarray(poses[i], np.float64)[:3, 3]], i
        assert d["map_points"] == len(before), i
        if stream == "built":
            # the map before followed by the reading as filtered, byte for byte
            kept_points = ctx.prefilter(raws[i])
            assert d["is_reference"] == 1 and run["states"][i]["count"] == 0 and run["kept"][i] == len(kept_points)
            before = np.concatenate([before, kept_points], 0)
        else:
            # no point is merged; the re-filter the rule asks for: count - 1 a multiple of map_refilter_every
            assert d["merged"] == 0 and run["states"][i]["count"] == i + 1 == run["states"][i]["n_processed"]
            assert d["refiltered"] == int(i % every == 0), i
            if d["refiltered"]:
                t = make_map(ctx, stream, before)
                t.prefilter()
                before = t.getCloud()
                t.free()
        assert run["maps"][i].tobytes() == before.tobytes(), i
    if stream == "prior":
        assert [d["refiltered"] for d in run["res"]] == [1, 0, 0, 0, 1, 0]


# ---- case 4: the gated append's edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4097])
def test_gated_append_edges(ctx, L, models, n):
    """An always-gating model (overlap < 1000) on pre-filtered entry, behind a 3001-point built map
    with no spare room (its tail starts off any block boundary): the prefix is unchanged, the tail is
    the reading's bytes, -0.0f and the subnormal included, and the size is exact."""
    from aicp_mapping_amd.built_map import BuiltMap
    from aicp_mapping_amd.map_session import MapSession

    full = scene_cloud(ORIGIN_A)
    mp = np.ascontiguousarray(full[np.linspace(0, len(full) - 1, 3001).astype(np.int64)])
    m = BuiltMap(ctx, mp)
    assert len(m) == m.capacity == 3001
    s = MapSession(ctx, m, params=L.default_built_map_params(reference_update_frequency=3),
                   risk=dict(model=models(("built", 1000.0))[0], threshold=0.5, params=risk_params(L)))
    s.start()
    P = edge_reading(n)
    pose = rr.pose(0.0, ORIGIN_B)
    T, d, kept, rec = s.process(P, pose)
    assert rec["registered"] == 0 and d["status"] == 0 and d["accepted"] == 1 and d["is_reference"] == 1 and kept == n
    assert d["map_points"] == 3001 and len(m) == 3001 + n and m.capacity >= 3001 + n
    got = m.getCloud()
    assert got[:3001].tobytes() == mp.tobytes()
    assert got[3001:].tobytes() == P.tobytes()
    st = s.state()
    assert st["count"] == 0 and np.array_equal(st["initial_T"], np.eye(4, dtype=F32))
    assert same_bits(d["corrected_origin"], pose[:3, 3], np.float64)
    if n == 4097:  # a smaller reading behind it lands at the new tail
        Q = edge_reading(255)
        T, d, kept, rec = s.process(Q, rr.pose(0.0, ORIGIN_A))
        assert rec["registered"] == 0 and kept == 255 and d["map_points"] == 3001 + n
        got = m.getCloud()
        assert len(got) == 3001 + n + 255 and got[:3001].tobytes() == mp.tobytes()
        assert got[3001:3001 + n].tobytes() == P.tobytes() and got[3001 + n:].tobytes() == Q.tobytes()
    s.close()
    m.free()


# ---- case 5: a dropped reading right after a gated one -----------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_dropped_reading_after_a_gated_one(ctx, L, worlds, models, stream):
    """max_correction_magnitude 0: every registered reading is dropped (on the prior map not the
    first of the graph), so a registered reading behind a gated one is dropped and changes nothing."""
    m = mid_window(ctx, L, worlds, models, stream, False, max_correction_magnitude=0.0)
    comp, run = m["comp"], m["run"]
    pairs = [i for i in range(1, len(comp)) if not comp[i - 1]["registered"] and comp[i]["registered"]]
    assert pairs and all(not comp[i]["accepted"] for i in pairs if stream == "built" or comp[i - 1]["count"] > 0)
    equals_loop(ctx, stream, run, comp, m["model"], m["ref_model"])
    for i in pairs:
        if run["res"][i]["accepted"]:
            continue
        assert run["states"][i]["count"] == run["states"][i - 1]["count"] and run["sizes"][i] == run["sizes"][i - 1]
        assert run["res"][i]["corrected_origin"] == [0.0, 0.0, 0.0] and run["res"][i][APPEND[stream]] == 0
    if stream == "prior" and not comp[0]["registered"]:  # the first-reading exemption ended at the gated first reading
        assert not any(c["accepted"] for c in comp if c["registered"])


# ---- case 6: readings from the sweep accumulator ---------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_readings_from_the_accumulator(ctx, L, models, stream):
    """process(acc, pose) reads the accumulator's cloud where it lies: the bits of a twin session on a
    twin map fed getCloud()'s rows; the accumulator is unchanged."""
    from aicp_mapping_amd.accumulator import SweepAccumulator

    def fill(acc, k):
        sweeps, poses = scene_sweeps(k)
        for sw, P in zip(sweeps, poses):
            acc.push(sw, P)
        return np.asarray(poses[1], np.float64)

    cap = max(sum(len(s) for s in scene_sweeps(k)[0]) for k in range(4))
    acc = SweepAccumulator(ctx, cap, batch_size=3)
    fill(acc, 0)
    first = ctx.prefilter(acc.getCloud())
    kw = dict(reference_update_frequency=2, max_correction_magnitude=1.0)
    golden = models("golden")[0]
    for thr in (1.0, 0.0):
        ma, mb = make_map(ctx, stream, first), make_map(ctx, stream, first)
        a, b = session(ctx, L, stream, ma, golden, thr, **kw), session(ctx, L, stream, mb, golden, thr, **kw)
        a.start()
        b.start()
        for k in (1, 2):
            acc.clear()
            P = fill(acc, k)
            cloud = acc.getCloud()
            Ta, ra, ka, qa = a.process(acc, P)
            assert same_bits(acc.getCloud(), cloud)
            Tb, rb, kb, qb = b.process(cloud, P)
            assert same_bits(Ta, Tb) and ra == rb and ka == kb and qa == qb, (thr, k)
            assert ra["status"] == 0 and qa["registered"] == int(thr == 1.0) and 50 <= ka < len(cloud)
            assert a.state()["count"] == b.state()["count"] and len(ma) == len(mb)
        assert same_bits(ma.getCloud(), mb.getCloud())
        for x in (a, b):
            x.close()
        for x in (ma, mb):
            x.free()
    acc.free()


# ---- case 7: isolation -----------------------------------------------------------------------------------
def test_other_calls_and_sessions_between_readings_change_nothing(ctx, L, worlds, models):
    """Other calls, a plain MapSession and an AppSession interleaved on the context: the built-map
    risk session's run in debug mode is its solo run."""
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.session import AppSession

    solo = mid_window(ctx, L, worlds, models, "built", True)
    pmp, praws, pposes, _ = worlds["prior"]
    pm = make_map(ctx, "prior", pmp)
    plain = MapSession(ctx, pm, params=params(L, "prior", False), prefilter=True)
    plain.start()
    st = sy.make_stream(n_readings=4, n_points=3000, seed=8, half=18.0)
    app = AppSession(ctx, params=L.default_sequence_params(reference_update_frequency=2))
    app.start(st.first, st.first_origin)
    other = sy.make_pair(3000, 3000, seed=5)

    def between(i, m):
        ctx.overlap(other.ref, other.read, other.ref_origin, other.read_origin)
        if i < len(praws):
            plain.process(praws[i], pposes[i])
        if i < 4:
            app.process(st.readings[i], st.origins[i])
        ctx.prefilter(praws[(i + 3) % len(praws)])
        if i % 2:
            ctx.register(other.ref, other.read)
        assert len(m.crop(-6.0, 6.0, worlds["built"][2][i])) > 0

    mp, raws, poses, _ = worlds["built"]
    run = feed(ctx, L, "built", mp, raws, poses, solo["model"], 0.5, True, between=between, **solo["kw"])
    same_run(run, solo["run"])
    plain.close()
    app.close()
    pm.free()


def same_run(a, b):
    assert a["rc"] == b["rc"] and len(a["res"]) == len(b["res"])
    for i in range(len(a["res"])):
        assert same_bits(a["T"][i], b["T"][i]) and a["res"][i] == b["res"][i] and a["kept"][i] == b["kept"][i], i
        assert a["rec"][i] == b["rec"][i] and a["sizes"][i] == b["sizes"][i], i
        assert a["states"][i]["count"] == b["states"][i]["count"], i
        assert same_bits(a["states"][i]["initial_T"], b["states"][i]["initial_T"]), i
    assert same_bits(a["final"], b["final"])


# ---- case 8: point-to-point chain ----------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_point_to_point_chain_equals_the_loop(ctx, L, worlds, models, stream):
    cfg = L.default_config(knn_normals=0)
    world, kw = worlds[stream], MID_KW[stream]
    n = len(world[1])
    X = mid_window(ctx, L, worlds, models, stream, False)["X"]  # (placed with the default chain; asserted below)
    model, ref_model = models((stream, X))
    comp = loop(ctx, L, stream, world, ref_model, 0.5, False, cfg=cfg, **kw)
    print(stream, "p2p features", [round(float(feature(stream, c)), 4) for c in comp], "X", X, "registered",
          [c["registered"] for c in comp])
    assert all(abs(feature(stream, c) - X) >= MARGIN[stream] for c in comp)
    assert {c["registered"] for c in comp} == {0, 1}
    assert any(c["registered"] and c["stats"]["iterations"] > 0 for c in comp)
    run = feed(ctx, L, stream, world[0], world[1][:n], world[2][:n], model, 0.5, False, cfg=cfg, **kw)
    equals_loop(ctx, stream, run, comp, model, ref_model)


# ---- case 9: the quality monitor ---------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_monitor_of_gated_and_registered_readings(ctx, L, worlds, models, stream):
    """A gated reading leaves valid = 0; a registered reading's monitor is the plain session's (up to
    the first gate the two sessions see the same maps)."""
    from aicp_mapping_amd.map_session import MapSession

    m = mid_window(ctx, L, worlds, models, stream, False)
    mp, raws, poses, _ = worlds[stream]
    run = feed(ctx, L, stream, mp, raws, poses, m["model"], 0.5, False, monitor=True, **m["kw"])
    same_run(run, m["run"])  # (the monitor changes no result)
    reg = [c["registered"] for c in m["comp"]]
    assert [q["valid"] for q in run["mon"]] == [bool(r) for r in reg]
    assert all(q["bytes"] == bytes(len(q["bytes"])) for q, r in zip(run["mon"], reg) if not r)

    def same_monitor(a, b):  # (the 56 bytes: a dict with a NaN in it never equals itself)
        return a["bytes"] == b["bytes"] and a["valid"] == b["valid"]

    first_gate = reg.index(0)
    tm = make_map(ctx, stream, mp)
    p = MapSession(ctx, tm, params=params(L, stream, False, **m["kw"]), prefilter=True, monitor=True)
    p.start()
    for i in range(first_gate):
        p.process(raws[i], poses[i])
        assert run["mon"][i]["valid"] and same_monitor(p.last_monitor(), run["mon"][i]), i
    if first_gate == 0:  # nothing to compare before the gate: the ungated session instead
        free = feed(ctx, L, stream, mp, raws[:2], poses[:2], models("golden")[0], 1.0, False, monitor=True, **m["kw"])
        for i in range(2):
            p.process(raws[i], poses[i])
            assert same_monitor(p.last_monitor(), free["mon"][i]) and free["mon"][i]["valid"], i
    p.close()
    tm.free()


# ---- case 10: endings ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crop", "emptied", "registration"])
@pytest.mark.parametrize("stream", STREAMS)
def test_what_ends_a_session(ctx, L, worlds, models, stream, kind):
    """The plain session's three endings, reached before the gate (the registration's behind it),
    then start."""
    mp, raws, poses, _ = worlds[stream]
    raws, poses = list(raws), list(poses)
    cfg = None
    if kind == "crop":
        far = np.array(poses[1], np.float64)
        far[:3, 3] += (200.0, 0.0, 0.0)
        poses[1] = far
    elif kind == "emptied":
        raws[1] = rs.scattered()
    else:  # nothing within nn_max_dist: no convergence. The crop still holds the map around the pose
        raws[1] = (raws[1] + F32([0.0, 0.0, 40.0])).astype(F32)
        cfg = L.default_config(nn_max_dist=5.0)
    m = make_map(ctx, stream, mp)
    s = session(ctx, L, stream, m, models("golden")[0], 1.0, False, cfg=cfg)
    s.start()
    T, d, k, rec = s.process(raws[0], poses[0])
    assert d["status"] == 0 and rec["registered"] == 1
    st0, map0 = s.state(), m.getCloud()
    T, d, k, rec = s.process(raws[1], poses[1], raise_on_error=False)
    err = ctx.last_error()
    assert d["rc"] == d["status"] != 0 and (d["rc"] == L.AICP_ERR_INVALID) == (kind != "registration")
    assert not d["accepted"] and not d[APPEND[stream]] and "reading 1" in err
    assert {"crop": "empty map crop", "emptied": "pre-filter", "registration": "status"}[kind] in err
    if kind != "registration":
        assert same_bits(T, np.eye(4, dtype=F32)) and d["crop_points"] == 0 and rec["registered"] == 0
    st1 = s.state()
    assert st1["ended"] and st1["n_processed"] == 2 and st1["count"] == st0["count"]
    assert same_bits(st1["initial_T"], st0["initial_T"]) and same_bits(m.getCloud(), map0)
    T, d, k, rec = s.process(raws[2], poses[2], raise_on_error=False)
    assert d["rc"] == L.AICP_ERR_INVALID and "ended at reading 1" in ctx.last_error()
    s.start()
    st2 = s.state()
    assert not st2["ended"] and st2["n_processed"] == 0 and st2["count"] == 0
    T, d, k, rec = s.process(raws[2], poses[2])
    assert d["status"] == 0 and s.state()["n_processed"] == 1
    s.close()
    m.free()


# ---- case 11: the handle kinds ----------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_handle_kinds_refuse_each_others_calls(ctx, L, worlds, models, stream):
    from aicp_mapping_amd.map_session import MapSession

    mp, raws, poses, _ = worlds[stream]
    m = make_map(ctx, stream, mp)
    risk = session(ctx, L, stream, m, models("golden")[0], 1.0)
    plain = MapSession(ctx, m, params=params(L, stream), prefilter=True)
    lib, bad = L.lib, L.AICP_ERR_INVALID
    c, keep = L.make_cloud(raws[0], np.asarray(poses[0], np.float64)[:3, 3])
    pz = np.ascontiguousarray(np.asarray(poses[0], F32).reshape(4, 4).T.reshape(16))
    pd = L._pose16(poses[0])
    res = (L.LocalizationResult if stream == "prior" else L.BuiltMapResult)()
    rec, kept = L.PipelineRecord(), C.c_uint32(9)
    for s in (risk, plain):
        s.start()
    T = np.full(16, 9.0, F32)
    assert lib.aicp_hip_map_session_process(ctx.h, risk.h, C.byref(c), L._fptr(pz), L._fptr(T), C.byref(res),
                                            C.byref(kept)) == bad
    assert "_risk" in ctx.last_error()
    assert lib.aicp_hip_map_session_process_accum(ctx.h, risk.h, None, L._fptr(pz), L._fptr(T), C.byref(res),
                                                  C.byref(kept)) == bad
    assert lib.aicp_hip_mapsession_process_risk(ctx.h, plain.h, C.byref(c), L._dptr(pd), L._fptr(T), C.byref(res),
                                                C.byref(rec), C.byref(kept)) == bad
    assert "create_risk" in ctx.last_error()
    for kw in (dict(pose=None), dict(rec=None), dict(out=None)):
        args = dict(pose=L._dptr(pd), rec=C.byref(rec), out=C.byref(res))
        args.update(kw)
        assert lib.aicp_hip_mapsession_process_risk(ctx.h, risk.h, C.byref(c), args["pose"], L._fptr(T), args["out"],
                                                    args["rec"], C.byref(kept)) == bad, kw
    assert (T == 9.0).all() and kept.value == 9 and res.map_points == 0 and len(m) == len(mp)
    assert same_bits(m.getCloud(), mp)
    for s in (risk, plain):
        st = s.state()
        assert st["n_processed"] == 0 and st["count"] == 0 and not st["ended"]
    # both still serve their own calls, and the shared ones (state, last_timing, the monitor's)
    T1, d1, k1, r1 = risk.process(raws[0], poses[0])
    assert d1["status"] == 0 and r1["registered"] == 1
    tm = risk.last_timing()
    assert 0 < tm["device_ms"] <= tm["wall_ms"]
    assert risk.last_monitor()["valid"] is False and risk.monitor_counters()["readings"] == 0
    for s in (risk, plain):
        s.close()
    m.free()


def test_create_refuses(ctx, L, models):
    cfg, loc, bmp, rp = L.default_config(), L.default_localization_params(), L.default_built_map_params(), \
        L.default_risk_params()
    model = models("golden")[0]
    bad, lib = L.AICP_ERR_INVALID, L.lib
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731

    def create(cfg_=cfg, loc_=loc, bm_=None, rp_=rp, model_=model.h, thr=0.5, pf_map=None):
        h = C.c_void_p(77)
        rc = lib.aicp_hip_mapsession_create_risk(ctx.h, ref(cfg_), ref(loc_), ref(bm_), None, ref(pf_map), ref(rp_),
                                                 model_, thr, C.byref(h))
        if rc == 0:
            lib.aicp_hip_map_session_free(ctx.h, h)
        else:
            assert h.value is None
        return rc

    assert create() == 0 and create(loc_=None, bm_=bmp) == 0
    assert create(bm_=bmp) == bad and create(loc_=None) == bad
    assert create(cfg_=None) == bad and create(rp_=None) == bad and create(model_=None) == bad
    assert create(thr=float("nan")) == bad
    assert create(loc_=None, bm_=bmp, pf_map=L.default_prefilter()) == bad
    # on the built map the overlap always runs: the flag may be left out, the resolution may not
    assert create(loc_=None, bm_=L.default_built_map_params(overlap=False)) == 0
    assert create(loc_=None, bm_=L.default_built_map_params(overlap=False, resolution=0.0)) == bad
    assert create(rp_=L.default_risk_params(prefilter=L.default_prefilter(normal_k=25))) == L.AICP_ERR_UNSUPPORTED


# ---- case 12: determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
def test_two_runs_are_identical(ctx, L, worlds, models, stream):
    m = mid_window(ctx, L, worlds, models, stream, True)
    mp, raws, poses, _ = worlds[stream]
    same_run(feed(ctx, L, stream, mp, raws, poses, m["model"], 0.5, True, **m["kw"]), m["run"])
