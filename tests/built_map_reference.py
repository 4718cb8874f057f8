"""App's localization stream on the map it has built itself (localize_against_built_map), restated
on the host from the oracle's building blocks only: crop_box, overlap, autotune_ratio, icp,
transform_cloud, corrected_origin, mul4 (oracle/pyoracle.py). The rules are the ones of
include/aicp_hip.h (aicp_hip_built_map_sequence_run), each with its App line:

  1. reference = getPointsInOrientedBox(map, crop_min, crop_max, prior pose as given)   app.cpp:60-69
     an empty crop is AICP_ERR_INVALID for that reading
  2. debug mode: reading = transformPointCloud(reading, initialT_), its origin = translation of
     initialT_ * prior pose                                                              app.cpp:87-96
  3. overlap(crop, translation of the pose as given, reading, its origin) -> autotune_ratio -> ICP
     (without the overlap: the chain's ratio); a non-zero status ends the stream   app.cpp:132-135, 210
  4. dropped when some |T(k,3)| > max_correction_magnitude, the first reading too      app.cpp:366-373
  5. accepted: corrected origin, ++acc; acc == reference_update_frequency: map += T * reading and
     acc = 0; initialT_ = correction * initialT_                          app.cpp:383-391, 414, 458-465
  6. the map is never re-filtered                                                        app.cpp:487

Also the fixture the CPU and GPU tests share, and the brute-force window simulation.
"""
import numpy as np

import localization_reference as lr

AICP_ERR_INVALID = 2


def replay(oracle, first_cloud, readings, poses, origins, cfg=None, reference_update_frequency=5,
           max_correction_magnitude=1.0, crop_min=-15.0, crop_max=15.0, resolution=0.2, overlap=True, debug=False,
           forced_T=None):
    """Returns (records, final map). forced_T (the device's corrections, 4x4 row-major each): every
    state update (the drop test, the count, corrected origin, initialT_, the append) uses
    forced_T[i] while the record still holds the replay's own T and statistics, so each reading is
    registered from the inputs the device had, bit for bit."""
    cfg = cfg or oracle.default_config()
    mp = np.ascontiguousarray(np.asarray(first_cloud, np.float32)[:, :3])
    mc = np.float32(max_correction_magnitude)
    acc = 0
    initT = np.eye(4, dtype=np.float32)
    out = []
    for i, (r, P, o) in enumerate(zip(readings, poses, origins)):
        rec = dict(status=0, accepted=0, is_reference=0, map_points=len(mp), crop_points=0, T=None, stats=None,
                   corrected_origin=None, overlap=-1.0, counts=None, ratio=None)
        out.append(rec)
        P32 = np.asarray(P, np.float32).reshape(4, 4)
        crop = oracle.crop_box(mp, crop_min, crop_max, P32)[0] if len(mp) else mp  # the pose as given
        rec["crop_points"] = len(crop)
        if len(crop) == 0:
            rec["status"] = AICP_ERR_INVALID
            break
        r = np.ascontiguousarray(np.asarray(r, np.float32)[:, :3])
        o = np.asarray(o, np.float64)
        if debug:
            r = oracle.transform_cloud(initT, r)
            o = oracle.corrected_origin(initT, o)
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


def simulate_windows(accept, freq, window):
    """App's counter over a given accept / drop sequence (accept[i]: reading i's correction passes
    the drop test), cut into windows by window(acc, remaining). Returns (window lengths, map-change
    indices, the indices of the changes that fall strictly inside a window: none are allowed)."""
    n = len(accept)
    acc = 0
    changes = []
    for i in range(n):
        if not accept[i]:
            continue
        acc += 1
        if acc == freq:
            changes.append(i)
            acc = 0
    wins, inside = [], []
    p = 0
    acc = 0
    while p < n:
        w = window(acc, n - p)
        assert 1 <= w <= n - p, (w, n - p)
        wins.append(w)
        inside += [c for c in changes if p <= c < p + w - 1]
        for i in range(p, p + w):
            if accept[i]:
                acc += 1
                if acc == freq:
                    acc = 0
        p += w
    return wins, changes, inside


# ---- the shared fixture ---------------------------------------------------------------------
PARAMS = dict(reference_update_frequency=3, max_correction_magnitude=0.4, crop_min=-6.0, crop_max=6.0, resolution=0.2)
JUMPS = {4: (0.0, -0.6, 0.0)}  # (not localization_reference.JUMPS: against the built map it leaves
JUMP_ON_0 = lr.JUMP_ON_0       # registrations that stop at the iteration limit)
N_READINGS = 10


def make_first_cloud(oracle):
    return lr.make_map(oracle)


def make_stream(n=N_READINGS, jumps=JUMPS):
    return lr.make_stream(n, jumps)
