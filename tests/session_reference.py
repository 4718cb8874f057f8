"""The live App session (aicp_hip_session_*, aicp_mapping_amd/session.py) restated as a host loop
over calls that existed before it, one pair at a time.

`replay` is App::processCloud in frame-to-reference mode (app.cpp:282-414) with
setAndFilterReading (app.cpp:77-100), reading after reading:

    debug mode: reading = transform(initialT_, reading), origin = corrected_origin(initialT_, origin)
    raw clouds: reading = prefilter(reading)
    overlap -> auto-tuned ratio -> ICP against the current reference         (one pair)
    some |t_i| > max_correction_magnitude: dropped, nothing changes
    accepted: the F-th since the last update becomes the reference: transform(T, reading) with
      origin corrected_origin(T, origin); initialT_ = mul4(T, initialT_)
    a registration error, or a reading the pre-filter empties, ends the loop

What does the three device steps comes in as a backend: `CtxBackend` uses the public calls of a
Context (prefilter, transform, align_batch of one pair with AICP_RUN_OVERLAP | AICP_RUN_ICP), so the
loop is the composition the session replaces; `OracleBackend` uses the CPU oracle's building
blocks, with which the loop must equal oracle.sequence record for record
(tests/test_session_cpu.py pins that). The host arithmetic (corrected_origin, mul4, the drop test)
is the oracle's in both.
"""
import numpy as np

ERR_INVALID = 2


class CtxBackend:
    def __init__(self, ctx, L, cfg=None, resolution=0.2, overlap=True, prefilter=None):
        self.ctx, self.L, self.cfg, self.res, self.ovl, self.pf = ctx, L, cfg, resolution, overlap, prefilter

    def prefilter(self, pts):
        return self.ctx.prefilter(pts, params=self.pf)

    def transform(self, T, pts):
        return self.ctx.transform(np.asarray(T, np.float32), np.ascontiguousarray(pts, np.float32))

    def align(self, ref, ref_origin, read, read_origin):
        L = self.L
        flags = L.AICP_RUN_ICP | (L.AICP_RUN_OVERLAP if self.ovl else 0)
        T, st, rc = self.ctx.align_batch([dict(ref=ref, read=read, ref_origin=ref_origin, read_origin=read_origin)],
                                         cfg=self.cfg, resolution=self.res, flags=flags, raise_on_error=False)
        s = st[0]
        return rc, T[0], dict(iterations=s["iterations"], counts=s["overlap_keys"], ratio=s["trimmed_ratio"], icp=s)


class OracleBackend:
    def __init__(self, oracle, cfg=None, resolution=0.2, overlap=True, prefilter=None):
        self.o, self.cfg, self.res, self.ovl = oracle, cfg or oracle.default_config(), resolution, overlap
        self.pf = prefilter or oracle.prefilter_params()

    def prefilter(self, pts):
        return self.o.prefilter(pts, self.pf)["out"]

    def transform(self, T, pts):
        return self.o.transform_cloud(T, pts)

    def align(self, ref, ref_origin, read, read_origin):
        o = self.o
        info = {}
        ratio = self.cfg.trimmed_ratio
        if self.ovl:
            ov, cnt = o.overlap(ref, ref_origin, read, read_origin, self.res)
            ratio = o.autotune_ratio(ov)
            info.update(overlap=ov, counts=[int(c) for c in cnt])
        c = o.IcpConfig.from_buffer_copy(self.cfg)
        c.trimmed_ratio = ratio
        rc, T, st = o.icp(ref, read, c)
        info.update(iterations=st.iterations, ratio=ratio, stats=st)
        return rc, T, info


def replay(backend, oracle, first, first_origin, readings, origins, freq=5, max_corr=1.0, debug=False, raw=False):
    """Returns (records, state). A record: status, T (4x4 row-major float32), accepted, reference,
    is_reference, corrected_origin, n_kept, registered (the reading as it was registered), prior_origin
    and the backend's info (iterations, counts, ratio, ...). state: reference, ref_origin, ref_id,
    initT, ended after the last record."""
    f32 = np.float32
    ref = backend.prefilter(first) if raw else np.ascontiguousarray(np.asarray(first, f32)[:, :3])
    ref_origin, ref_id = np.asarray(first_origin, np.float64), -1
    initT = np.eye(4, dtype=f32)
    acc, out, ended = 0, [], False
    mc = f32(max_corr)
    for i, (r, o) in enumerate(zip(readings, origins)):
        r = np.ascontiguousarray(np.asarray(r, f32)[:, :3])
        o = np.asarray(o, np.float64)
        if debug:
            r = backend.transform(initT, r)
            o = oracle.corrected_origin(initT, o)
        if raw:
            r = backend.prefilter(r)
        rec = dict(reference=ref_id, is_reference=0, accepted=0, corrected_origin=None, prior_origin=o,
                   n_kept=len(r), registered=r, T=np.eye(4, dtype=f32))
        out.append(rec)
        if len(r) == 0:
            rec["status"] = ERR_INVALID
            ended = True
            break
        rc, T, info = backend.align(ref, ref_origin, r, o)
        rec.update(info)
        rec.update(status=rc, T=np.asarray(T, f32))
        if rc:
            ended = True
            break
        Tf = rec["T"]
        if any(abs(Tf[k, 3]) > mc for k in range(3)):
            continue
        rec["accepted"] = 1
        rec["corrected_origin"] = oracle.corrected_origin(Tf, o)
        acc += 1
        if acc == freq:
            ref, ref_origin, ref_id = backend.transform(Tf, r), rec["corrected_origin"], i
            rec["is_reference"] = 1
            acc = 0
        initT = oracle.mul4(Tf, initT)
    return out, dict(reference=ref, ref_origin=ref_origin, ref_id=ref_id, initT=initT, ended=ended)
