"""The two map localization streams on RAW readings (aicp_hip_map_sequence_run_raw,
aicp_hip_built_map_sequence_run_raw), restated on the host from the oracle's building blocks only:
crop_box, transform_cloud, prefilter, overlap, autotune_ratio, icp, corrected_origin, mul4
(oracle/pyoracle.py). Every rule is the one of tests/localization_reference.py /
tests/built_map_reference.py; only the reading differs (setAndFilterReading, app.cpp:77-100):

  robot mode:  reading = prefilter(raw)                                              app.cpp:87-88
  debug mode:  reading = prefilter(transformPointCloud(raw, initialT_)), prior pose =
               initialT_ * prior pose; the filtered reading is not moved again       app.cpp:90-99
  a reading the pre-filter empties is AICP_ERR_INVALID and ends the stream (libpointmatcher throws
  on an empty cloud); it is looked at before the reading's crop
  the map append takes the filtered reading (App's read_prefiltered)

order="swapped" is the other order, filter-then-move (what the pre-filtered streams' debug flag
does to a cloud filtered beforehand): prefilter(raw) moved by initialT_. The 0.08 m VoxelGrid is
aligned to the world frame, so the two orders keep different points unless initialT_ is the
identity.

Also the fixtures the CPU and GPU tests share.
"""
import numpy as np

import built_map_reference as bm
import localization_reference as lr

AICP_ERR_INVALID = 2


def _reading(oracle, raw, origin, initT, debug, order, pf):
    """setAndFilterReading: (the filtered reading, its sensor origin)."""
    raw = np.ascontiguousarray(np.asarray(raw, np.float32)[:, :3])
    o = np.asarray(origin, np.float64)
    if not debug:
        return oracle.prefilter(raw, pf)["out"], o
    o = oracle.corrected_origin(initT, o)
    if order == "app":
        return oracle.prefilter(oracle.transform_cloud(initT, raw), pf)["out"], o
    assert order == "swapped", order
    kept = oracle.prefilter(raw, pf)["out"]
    return (oracle.transform_cloud(initT, kept) if len(kept) else kept), o


def replay_prior_raw(oracle, map_pts, raws, poses, origins, cfg=None, reference_update_frequency=5,
                     map_refilter_every=30, max_correction_magnitude=1.0, crop_min=-15.0, crop_max=15.0, merge=True,
                     debug=False, prefilter_params=None, read_prefilter=None, forced_T=None, order="app"):
    """Returns (records, final map); records as localization_reference.replay's plus `kept`.
    forced_T as there: every state update uses forced_T[i]."""
    cfg = cfg or oracle.default_config()
    mp = np.ascontiguousarray(np.asarray(map_pts, np.float32)[:, :3])
    mc = np.float32(max_correction_magnitude)
    n_clouds = 0
    initT = np.eye(4, dtype=np.float32)
    out = []
    for i, (raw, P, o) in enumerate(zip(raws, poses, origins)):
        rec = dict(status=0, accepted=0, merged=0, refiltered=0, map_points=len(mp), crop_points=0, T=None,
                   stats=None, corrected_origin=None, kept=0)
        out.append(rec)
        r, o = _reading(oracle, raw, o, initT, debug, order, read_prefilter)
        rec["kept"] = len(r)
        if len(r) == 0:
            rec["status"] = AICP_ERR_INVALID
            break
        crop = oracle.crop_box(mp, crop_min, crop_max, P)[0] if len(mp) else mp  # the pose as given
        rec["crop_points"] = len(crop)
        if len(crop) == 0:
            rec["status"] = AICP_ERR_INVALID
            break
        c = type(cfg).from_buffer_copy(cfg)
        c.trimmed_ratio = oracle.autotune_ratio(50.0)
        rc, T, st = oracle.icp(crop, r, c)
        rec.update(status=rc, T=T, stats=st)
        if rc:
            break
        Tu = np.asarray(T if forced_T is None else forced_T[i], np.float32)
        if n_clouds != 0 and any(abs(Tu[k, 3]) > mc for k in range(3)):
            continue
        n_clouds += 1
        rec["accepted"] = 1
        rec["corrected_origin"] = oracle.corrected_origin(Tu, o)
        initT = oracle.mul4(Tu, initT)
        if merge and (n_clouds - 1) % reference_update_frequency == 0:
            mp = np.concatenate([mp, oracle.transform_cloud(Tu, r)], 0)
            rec["merged"] = 1
        if merge and map_refilter_every > 0 and (n_clouds - 1) % map_refilter_every == 0:
            mp = oracle.prefilter(mp, prefilter_params)["out"]
            rec["refiltered"] = 1
    return out, mp


def replay_built_raw(oracle, first_cloud, raws, poses, origins, cfg=None, reference_update_frequency=5,
                     max_correction_magnitude=1.0, crop_min=-15.0, crop_max=15.0, resolution=0.2, overlap=True,
                     debug=False, read_prefilter=None, forced_T=None, order="app"):
    """Returns (records, final map); records as built_map_reference.replay's plus `kept`."""
    cfg = cfg or oracle.default_config()
    mp = np.ascontiguousarray(np.asarray(first_cloud, np.float32)[:, :3])
    mc = np.float32(max_correction_magnitude)
    acc = 0
    initT = np.eye(4, dtype=np.float32)
    out = []
    for i, (raw, P, o) in enumerate(zip(raws, poses, origins)):
        rec = dict(status=0, accepted=0, is_reference=0, map_points=len(mp), crop_points=0, T=None, stats=None,
                   corrected_origin=None, overlap=-1.0, counts=None, ratio=None, kept=0)
        out.append(rec)
        r, o = _reading(oracle, raw, o, initT, debug, order, read_prefilter)
        rec["kept"] = len(r)
        if len(r) == 0:
            rec["status"] = AICP_ERR_INVALID
            break
        P32 = np.asarray(P, np.float32).reshape(4, 4)
        crop = oracle.crop_box(mp, crop_min, crop_max, P32)[0] if len(mp) else mp  # the pose as given
        rec["crop_points"] = len(crop)
        if len(crop) == 0:
            rec["status"] = AICP_ERR_INVALID
            break
        c = type(cfg).from_buffer_copy(cfg)
        if overlap:
            ov, cnt = oracle.overlap(crop, P32[:3, 3].astype(np.float64), r, o, resolution)
            c.trimmed_ratio = oracle.autotune_ratio(ov)
            rec.update(overlap=ov, counts=[int(x) for x in cnt])
        rec["ratio"] = np.float32(c.trimmed_ratio)
        rc, T, st = oracle.icp(crop, r, c)
        rec.update(status=rc, T=T, stats=st)
        if rc:
            break
        Tu = np.asarray(T if forced_T is None else forced_T[i], np.float32)
        if any(abs(Tu[k, 3]) > mc for k in range(3)):
            continue
        rec["accepted"] = 1
        rec["corrected_origin"] = oracle.corrected_origin(Tu, o)
        acc += 1
        if acc == reference_update_frequency:
            mp = np.concatenate([mp, oracle.transform_cloud(Tu, r)], 0)
            rec["is_reference"] = 1
            acc = 0
        initT = oracle.mul4(Tu, initT)
    return out, mp


# ---- the shared fixtures --------------------------------------------------------------------
N_RAW = 6000      # raw points per reading (the pre-filter keeps 5120-5204 of them in robot mode)
N_PRIOR = 8
N_BUILT = 10
# built map: with built_map_reference.JUMPS no reading is dropped at 6000 raw points. This jump
# (a vertical one) makes the replay alone drop reading 3 in both modes and still append readings
# 2, 6 and 9 (test_raw_stream_cpu.py asserts it)
BUILT_JUMPS = {3: (0.0, 0.0, 0.6)}


def _stream(n, jumps):
    rd = [lr.make_reading(i, n_points=N_RAW, jump=jumps.get(i)) for i in range(n)]
    raws, poses = [r[0] for r in rd], [r[1] for r in rd]
    return raws, poses, [p[:3, 3].copy() for p in poses]


def prior_world(oracle):
    """(map, raw readings, poses, origins) of the prior-map fixture; parameters: lr.PARAMS."""
    return (lr.make_map(oracle),) + _stream(N_PRIOR, lr.JUMPS)


def built_world(oracle):
    """(first cloud, raw readings, poses, origins) of the built-map fixture; parameters: bm.PARAMS."""
    return (bm.make_first_cloud(oracle),) + _stream(N_BUILT, BUILT_JUMPS)


def scattered(n=30, seed=11):
    """n points more than a metre apart: no cluster reaches the pre-filter's minimum size, so it
    keeps none of them."""
    g = np.random.default_rng(seed)
    idx = g.permutation(64)[:n]
    grid = np.stack([idx % 4, (idx // 4) % 4, idx // 16], 1).astype(np.float32)
    return (grid * np.float32(2.5) + g.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)).astype(np.float32)
