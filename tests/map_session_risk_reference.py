"""App's two map localization policies with failure_prediction_mode, as a host loop over public
one-reading calls (the pattern of tests/session_risk_reference.py), and the policies' bookkeeping
without any cloud (MapGatePolicy). The rules are those of include/aicp_hip.h at
aicp_hip_mapsession_create_risk (app.cpp:236-245, 362-414, 458-493):

  crop at the prior pose P cast to float; the features' reference pose is P as given
  reading = prefilter(raw), debug mode: prefilter(transform(initialT_, raw)) with the pose
            fromMatrix4fToIsometry3d(initialT_) * P
  overlap: prior map 50.0; built map the octree overlap of (crop, reading), origins: the float
           pose's translation and the reading pose's
  gated = !(risk(overlap, alignability) <= threshold); ratio = autotune(overlap)
  not gated: ICP at that ratio, then the policy's rules as tests/raw_stream_reference.py states them
  gated: identity correction, initialT_ stays, no drop test, accepted; built map: map += the
         reading's bytes, count = 0; prior map: ++count, no merge, the re-filter test still applies

The loop keeps the map on the host and puts it on the device for every reading (a PriorMap /
BuiltMap of its own), so that the crop and the registration are the library's one-reading calls.
"""
import numpy as np

import svm_reference as sr

F32 = np.float32
AICP_ERR_INVALID = 2


class MapGatePolicy:
    """count (prior map: the clouds in the graph; built map: accepted since the last reference) and
    initialT_. step() takes one reading's risk and correction and returns its flags."""

    def __init__(self, built, frequency, max_correction, threshold, refilter_every=0, merge=True):
        self.built, self.F, self.max_corr, self.thr = bool(built), int(frequency), F32(max_correction), float(threshold)
        self.every, self.merge = int(refilter_every), bool(merge)
        self.count = 0
        self.initT = np.eye(4, dtype=F32)

    def gated(self, risk):
        return not (risk <= self.thr)

    def step(self, risk, T):
        """T: the correction (4x4 float32; ignored for a gated reading). Returns dict(registered,
        accepted, append, refilter)."""
        out = dict(registered=0, accepted=0, append=0, refilter=0)
        if self.gated(risk):  # app.cpp:401-411: the correction is the identity, initialT_ stays
            out["accepted"] = 1
            if self.built:  # the reading is the reference at once
                self.count = 0
                out["append"] = 1
            else:  # marked a reference: app.cpp:469-483 is not reached, app.cpp:487-493 is
                self.count += 1
                out["refilter"] = int(self.merge and self.every > 0 and (self.count - 1) % self.every == 0)
            return out
        out["registered"] = 1
        T = np.asarray(T, F32)
        if (self.built or self.count != 0) and (np.abs(T[:3, 3]) > self.max_corr).any():  # app.cpp:366-373
            return out
        out["accepted"] = 1
        self.count += 1
        self.initT = sr.mul4f(T, self.initT)  # app.cpp:414
        if self.built:
            if self.count == self.F:  # app.cpp:383-391
                out["append"] = 1
                self.count = 0
        elif self.merge:
            out["append"] = int((self.count - 1) % self.F == 0)
            out["refilter"] = int(self.every > 0 and (self.count - 1) % self.every == 0)
        return out


class CtxBlocks:
    """The loop's building blocks from a Context's public calls and the numpy classifier."""

    def __init__(self, ctx, L, ref_model, built, prm, risk_params, cfg=None, prefilter=True):
        """prm: dict(crop_min, crop_max, resolution (built map))."""
        self.ctx, self.L, self.model, self.built, self.prm, self.rp = ctx, L, ref_model, built, prm, risk_params
        self.cfg, self.pf = cfg or L.default_config(), prefilter

    def prefilter(self, cloud):
        return self.ctx.prefilter(cloud) if self.pf else np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])

    def transform(self, T, cloud):
        return self.ctx.transform(T, cloud)

    def device_map(self, pts):
        from aicp_mapping_amd.built_map import BuiltMap
        from aicp_mapping_amd.prior_map import PriorMap

        return (BuiltMap if self.built else PriorMap)(self.ctx, pts)

    def crop(self, m, P32):
        return m.crop(self.prm["crop_min"], self.prm["crop_max"], P32)

    def overlap(self, crop, read, o_crop, o_read):
        """(percent, keys) of the one-pair overlap call."""
        _, st, rc = self.ctx.align_batch([dict(ref=crop, read=read, ref_origin=o_crop, read_origin=o_read)],
                                         cfg=self.cfg, flags=self.L.AICP_RUN_OVERLAP, resolution=self.prm["resolution"])
        assert rc == 0
        return st[0]["overlap_percent"], st[0]["overlap_keys"]

    def features(self, crop, read, crop_pose, read_pose):
        return self.ctx.alignment_features(crop, read, crop_pose, read_pose, self.rp)

    def classify(self, overlap, alignability):
        raw, risk, _ = sr.predict(self.model, np.array([[overlap, alignability]], F32))
        return raw[0], risk[0]

    def register(self, m, read, P32, ratio):
        """The map's one-reading registration at `ratio`: (T, stats)."""
        mn, mx = self.prm["crop_min"], self.prm["crop_max"]
        if self.built:
            c = type(self.cfg).from_buffer_copy(self.cfg)
            c.trimmed_ratio = ratio
            T, st, rc = m.align_batch([read], [P32], mn, mx, cfg=c, flags=0)
        else:  # (the call tunes the ratio from the constant 50 itself)
            T, st, rc = m.register_batch([read], [P32], mn, mx, cfg=self.cfg)
        assert rc == 0
        return T[0], st[0]


def host_loop(blocks, map_pts, readings, poses, frequency, max_corr, threshold, debug, refilter_every=0, merge=True,
              map_prefilter=None):
    """One dict per reading: MapGatePolicy.step's flags, T, stats (None for a gated reading), kept,
    map_points, crop_points, overlap, keys, fov_overlap, alignability, raw, risk, ratio,
    corrected_origin (None for a dropped reading), and after the reading: count, initial_T, map (the
    host copy). An emptied reading or an empty crop ends the loop with status AICP_ERR_INVALID."""
    L, built = blocks.L, blocks.built
    mp = np.ascontiguousarray(np.asarray(map_pts, F32)[:, :3])
    policy = MapGatePolicy(built, frequency, max_corr, threshold, refilter_every, merge)
    out = []
    for cloud, pose in zip(readings, poses):
        P = np.asarray(pose, np.float64).reshape(4, 4)
        P32 = P.astype(F32)
        d = dict(status=0, registered=0, accepted=0, append=0, refilter=0, T=np.eye(4, dtype=F32), stats=None, kept=0,
                 map_points=len(mp), crop_points=0, corrected_origin=None)
        out.append(d)
        prior = sr.moved_pose(policy.initT, P) if debug else P.copy()
        rd = blocks.prefilter(blocks.transform(policy.initT, cloud) if debug else cloud)
        d["kept"] = len(rd)
        if len(rd) == 0:
            d["status"] = AICP_ERR_INVALID
            break
        m = blocks.device_map(mp)
        try:
            crop = blocks.crop(m, P32)
            d["crop_points"] = len(crop)
            if len(crop) == 0:
                d["status"] = AICP_ERR_INVALID
                break
            ov, keys = (blocks.overlap(crop, rd, P32[:3, 3].astype(np.float64), prior[:3, 3]) if built
                        else (50.0, [0, 0, 0]))
            f = blocks.features(crop, rd, P, prior)
            raw, risk = blocks.classify(ov, f["alignability"])
            ratio = L.autotune_ratio(float(F32(ov)))
            d.update(overlap=ov, keys=keys, fov_overlap=f["fov_overlap"], alignability=f["alignability"], raw=raw,
                     risk=risk, ratio=ratio)
            T = np.eye(4, dtype=F32)
            if not policy.gated(risk):
                T, d["stats"] = blocks.register(m, rd, P32, ratio)
            d.update(policy.step(risk, T), T=np.asarray(T, F32))
            if not d["registered"]:
                d["corrected_origin"] = prior[:3, 3].copy()
                if d["append"]:  # the bytes (apply4 by the identity would lose -0.0f)
                    mp = np.concatenate([mp, rd], 0)
            elif d["accepted"]:
                d["corrected_origin"] = sr.moved_pose(T, prior)[:3, 3].copy()
                if d["append"]:
                    m.merge(rd, T)
                    mp = m.getCloud()
            if d["refilter"]:
                m.prefilter(map_prefilter)
                mp = m.getCloud()
        finally:
            m.free()
        d.update(count=policy.count, initial_T=policy.initT.copy(), map=mp)
    return out
