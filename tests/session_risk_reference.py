"""App's frame-to-reference stream with failure_prediction_mode as a host loop over building blocks:
compose() of tests/test_risk_pipeline.py with a configurable chain and max_correction_magnitude,
which also returns the reference, its pose and initialT_ after every reading. The policy is
svm_reference.GatePolicy, the poses svm_reference.moved_pose / fix_pitch_roll.

The blocks are an object with
    prefilter(cloud) -> kept points            transform(T, cloud) -> moved cloud
    overlap(ref, read, o_ref, o_read) -> %     alignability(ref, read, ref_pose, read_pose) -> float
    risk(overlap, alignability) -> float       register(ref, read, o_ref, o_read) -> (T, iterations)
CtxBlocks serves them from a Context's public one-pair calls and the numpy classifier;
tests/test_session_risk_cpu.py passes stand-ins."""
import numpy as np

import svm_reference as sr

F32 = np.float32


def apply4(T, P):
    """pcl::transformPointCloud as the library does it: float, term by term, no FMA."""
    T, P = np.asarray(T, F32), np.asarray(P, F32)
    out = np.empty_like(P)
    for r in range(3):
        s = T[r, 0] * P[:, 0]
        s = s + T[r, 1] * P[:, 1]
        s = s + T[r, 2] * P[:, 2]
        out[:, r] = s + T[r, 3]
    return out


class CtxBlocks:
    def __init__(self, ctx, L, ref_model, resolution, risk_params, cfg=None, prefilter=True):
        self.ctx, self.L, self.model, self.res, self.rp, self.cfg = ctx, L, ref_model, resolution, risk_params, cfg
        self.pf = prefilter

    def prefilter(self, cloud):
        return self.ctx.prefilter(cloud) if self.pf else np.ascontiguousarray(cloud, F32)

    def transform(self, T, cloud):
        return self.ctx.transform(T, cloud)

    def overlap(self, ref, read, o_ref, o_read):
        return self.ctx.overlap(ref, read, o_ref, o_read, self.res)

    def alignability(self, ref, read, ref_pose, read_pose):
        return self.ctx.alignment_features(ref, read, ref_pose, read_pose, self.rp)["alignability"]

    def risk(self, overlap, alignability):
        return sr.predict(self.model, np.array([[overlap, alignability]], F32))[1][0]

    def register(self, ref, read, o_ref, o_read):
        L = self.L
        Ts, sts, rc = self.ctx.align_batch([dict(ref=ref, read=read, ref_origin=o_ref, read_origin=o_read)],
                                           cfg=self.cfg, flags=L.AICP_RUN_OVERLAP | L.AICP_RUN_ICP,
                                           resolution=self.res)
        assert rc == 0
        return Ts[0], sts[0]["iterations"]


def host_loop(blocks, first, first_pose, readings, poses, freq, max_corr, threshold, debug):
    """One dict per reading: GatePolicy.step's flags, T, overlap, alignability, risk, kept,
    iterations, corrected_origin (None for a dropped reading), and after the reading: ref (the
    reference's points), ref_pose (4x4 float64), initial_T (4x4 float32)."""
    ref = blocks.prefilter(first)
    ref_pose = sr.fix_pitch_roll(first_pose, first_pose)
    policy = sr.GatePolicy(freq, max_corr, threshold)
    out = []
    for i, (cloud, odom) in enumerate(zip(readings, poses)):
        odom = np.asarray(odom, np.float64)
        prior = sr.moved_pose(policy.initT, odom) if debug else odom.copy()
        rd = blocks.prefilter(blocks.transform(policy.initT, cloud) if debug else cloud)
        ov = blocks.overlap(ref, rd, ref_pose[:3, 3], prior[:3, 3])
        al = blocks.alignability(ref, rd, ref_pose, prior)
        risk = blocks.risk(ov, al)
        T, iters = np.eye(4, dtype=F32), 0
        if not policy.gated(risk):
            T, iters = blocks.register(ref, rd, ref_pose[:3, 3], prior[:3, 3])
        d = policy.step(i, risk, T)
        d.update(T=np.asarray(T, F32), overlap=ov, alignability=al, risk=risk, kept=len(rd), iterations=iters,
                 corrected_origin=None)
        if not d["registered"]:  # app.cpp:401-411
            d["corrected_origin"] = prior[:3, 3].copy()
            ref, ref_pose = rd, sr.fix_pitch_roll(prior, odom)
        elif d["accepted"]:
            corrected = sr.moved_pose(T, prior)
            d["corrected_origin"] = corrected[:3, 3].copy()
            if d["is_reference"]:  # app.cpp:375-391
                ref, ref_pose = apply4(T, rd), sr.fix_pitch_roll(corrected, odom)
        d.update(ref=ref, ref_pose=ref_pose.copy(), initial_T=policy.initT.copy())
        out.append(d)
    return out
