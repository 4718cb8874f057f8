"""The mapping session's built map, the go-back and the start on a loaded map, as host loops over
public calls (the pattern of tests/session_reference.py and tests/map_session_risk_reference.py).

  drive            one AppSession over a start and a list of process calls; with keeping off the
                   aligned map is formed on the host: the first cloud's reference() and, after
                   every call whose result says is_reference, the new reference(), concatenated
                   (app.cpp:310, 458-468)
  GoBackCount      App's graph count as a state machine (getNbClouds(): the first cloud, the
                   accepted readings, gated ones included), and the same count from a brute-force
                   graph (a list of clouds)
  go_back_loop     App on the prior map from a given n_clouds and initialT_, one reading per turn
                   over PriorMap.crop / register_batch / merge / prefilter, rules 1-7 of
                   tests/localization_reference.py
  on_map_loop      load_map_from_file without localising: the crop at the pose is the reference,
                   the first reading through a plain session of frequency 1 and a huge
                   max_correction_magnitude, the rest through a plain session started on the
                   promoted reference, initialT_ carried by the host's float product
"""
import numpy as np

import svm_reference as sv

F32 = np.float32
AICP_ERR_INVALID = 2
HUGE = 1.0e30  # a max_correction_magnitude no correction reaches


def same_bits(a, b, dtype=F32):
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def strip(res):
    return {k: v for k, v in res.items() if k != "rc"}


def drive(s, start, steps, keep, on_map=False):
    """start(): the session's start; steps: callables, each one process call returning the
    session's tuple (raise_on_error False). keep: the session keeps its aligned map and maps[i] is
    its content after call i; otherwise maps[i] is the host's concatenation of reference().
    Returns dict(T, out, kept, extra (the tuple's tail), states, refs, maps, map0)."""
    start()
    host = np.zeros((0, 3), F32) if on_map else s.reference()[0]
    run = dict(T=[], out=[], kept=[], extra=[], states=[], refs=[], maps=[], caps=[],
               map0=s.aligned_map.getCloud() if keep else host)
    for step in steps:
        r = step()
        T, res, kept = r[:3]
        run["T"].append(T)
        run["out"].append(strip(res))
        run["kept"].append(kept)
        run["extra"].append(r[3:])
        run["states"].append(s.state())
        run["refs"].append(s.reference())
        if keep:
            m = s.aligned_map
            run["maps"].append(m.getCloud())
            run["caps"].append(m.capacity)
        else:
            if res["rc"] == 0 and res["is_reference"]:
                host = np.concatenate([host, run["refs"][-1][0]], 0)
            run["maps"].append(host)
        if res["rc"]:
            break
    return run


def same_outputs(a, b):
    """Everything a caller sees of two driven runs but the map: every bit."""
    assert len(a["T"]) == len(b["T"])
    for i in range(len(a["T"])):
        assert same_bits(a["T"][i], b["T"][i]), i
        assert a["out"][i] == b["out"][i], i
        assert a["kept"][i] == b["kept"][i], i
        assert a["extra"][i] == b["extra"][i], i
        sa, sb = dict(a["states"][i]), dict(b["states"][i])
        assert same_bits(sa.pop("initial_T"), sb.pop("initial_T")) and sa == sb, i
        assert same_bits(a["refs"][i][0], b["refs"][i][0]) and np.array_equal(a["refs"][i][1], b["refs"][i][1]), i


def same_maps(a, b):
    assert same_bits(a["map0"], b["map0"])
    assert len(a["maps"]) == len(b["maps"])
    for i, (x, y) in enumerate(zip(a["maps"], b["maps"])):
        assert same_bits(x, y), (i, len(x), len(y))


# ---- the go-back's count ------------------------------------------------------------------------
class GoBackCount:
    """aligned_clouds_graph_->getNbClouds() of a frame-to-reference App as the library counts it:
    1 for the first cloud (0 after a start on a map) plus the accepted readings. events: "a"
    accepted, "d" dropped, "g" gated (accepted unmoved), "e" the reading that ends the worker."""

    def __init__(self, on_map=False):
        self.on_map, self.accepted, self.ended = on_map, 0, False

    def step(self, event):
        assert not self.ended
        if event in ("a", "g"):
            self.accepted += 1
        elif event == "e":
            self.ended = True
        else:
            assert event == "d"

    @property
    def n_clouds(self):
        return (0 if self.on_map else 1) + self.accepted


def brute_force_graph(events, on_map=False):
    """App's graph as a list: initialiseCloud adds the first cloud (app.cpp:293-310), every accepted
    reading is added (app.cpp:375-399), a gated one too (app.cpp:401-411); a dropped reading and
    the reading that kills the worker add nothing."""
    graph = [] if on_map else ["first"]
    for i, e in enumerate(events):
        if e == "e":
            break
        if e in ("a", "g"):
            graph.append(i)
    return len(graph)


def go_back_loop(ctx, L, map_pts, readings, poses, n_clouds, initT, freq, refilter_every, max_corr, crop, cfg=None,
                 merge=True, map_prefilter=None):
    """Returns (records, final map, n_clouds, initialT_). A record: status, accepted, merged,
    refiltered, map_points, crop_points, T, icp (None when nothing was registered),
    corrected_origin ([0, 0, 0] for a dropped reading). Robot mode, pre-filtered readings."""
    from aicp_mapping_amd.prior_map import PriorMap

    m = PriorMap(ctx, map_pts)
    mc = F32(max_corr)
    initT = np.asarray(initT, F32).copy()
    out = []
    try:
        for r, P in zip(readings, poses):
            P = np.asarray(P, np.float64).reshape(4, 4)
            rec = dict(status=0, accepted=0, merged=0, refiltered=0, map_points=len(m), crop_points=0,
                       T=np.eye(4, dtype=F32), icp=None, corrected_origin=[0.0, 0.0, 0.0])
            out.append(rec)
            rec["crop_points"] = len(m.crop(-crop, crop, P.astype(F32)))  # 1.
            if rec["crop_points"] == 0:
                rec["status"] = AICP_ERR_INVALID
                break
            T, st, rc = m.register_batch([r], [P], -crop, crop, cfg=cfg)  # 3. (the ratio of 50 is the call's)
            rec.update(status=rc, T=np.asarray(T[0], F32), icp=st[0])
            if rc:
                break
            Tu = rec["T"]
            if n_clouds != 0 and any(abs(Tu[k, 3]) > mc for k in range(3)):  # 4.
                continue
            n_clouds += 1  # 5.
            rec["accepted"] = 1
            rec["corrected_origin"] = [float(x) for x in sv.moved_pose(Tu, P)[:3, 3]]
            initT = sv.mul4f(Tu, initT)
            if merge and (n_clouds - 1) % freq == 0:  # 6.
                m.merge(r, Tu)
                rec["merged"] = 1
            if merge and refilter_every > 0 and (n_clouds - 1) % refilter_every == 0:  # 7.
                m.prefilter(map_prefilter)
                rec["refiltered"] = 1
        return out, m.getCloud(), n_clouds, initT
    finally:
        m.free()


def on_map_loop(ctx, L, map_pts, pose, crop, readings, origins, freq, max_corr, debug, cfg=None, resolution=0.2):
    """Returns (records, maps): per reading T, out (the result with `reference` in the numbering of
    one session: -1, then the call's index), initial_T after it and the reference after it; maps[i]:
    the aligned map after reading i (no first cloud: the promoted references alone). Pre-filtered
    readings; debug: the readings moved by the carried initialT_ on the host."""
    from aicp_mapping_amd.prior_map import PriorMap
    from aicp_mapping_amd.session import AppSession

    def prm(f, mc):
        return L.default_sequence_params(reference_update_frequency=f, max_correction_magnitude=mc, resolution=resolution,
                                         flags=L.AICP_RUN_OVERLAP)

    pose = np.asarray(pose, np.float64).reshape(4, 4)
    m = PriorMap(ctx, map_pts)
    ref = m.crop(-crop, crop, pose.astype(F32))
    m.free()
    assert len(ref)
    origin = pose.astype(F32)[:3, 3].astype(np.float64)
    initT = np.eye(4, dtype=F32)
    recs, maps, amap = [], [], np.zeros((0, 3), F32)
    s = AppSession(ctx, cfg=cfg, params=prm(1, HUGE))  # the first reading: no drop test, promoted
    s.start(ref, origin)
    base = 0  # the index of the second session's first reading
    for i, (r, o) in enumerate(zip(readings, origins)):
        o = np.asarray(o, np.float64)
        if debug:
            at = np.eye(4)
            at[:3, 3] = o
            r, o = ctx.transform(initT, r), sv.moved_pose(initT, at)[:3, 3]
        T, res, kept = s.process(r, o)
        out = strip(res)
        if i >= base and base:  # the second session numbers its readings from 0 and its start -1
            out["reference"] = out["reference"] + base if out["reference"] >= 0 else base - 1
        if out["accepted"]:
            initT = sv.mul4f(T, initT)
        pts, org = s.reference()
        if out["is_reference"]:
            amap = np.concatenate([amap, pts], 0)
        recs.append(dict(T=T, out=out, kept=kept, initial_T=initT.copy(), ref=(pts, org)))
        maps.append(amap)
        if i == 0:
            assert out["accepted"] and out["is_reference"]
            s.close()
            s = AppSession(ctx, cfg=cfg, params=prm(freq, max_corr))
            s.start(pts, org)
            base = 1
    s.close()
    return recs, maps
