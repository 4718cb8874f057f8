"""Live App session: App::processCloud, one reading per call, with App's state on the device.

The reference node never sees a recording: ``AppROS::velodyneCallBack`` assembles one reading and
``App::processCloud`` (app.cpp:282-414) handles it against the state it keeps between calls, the
current reference, ``initialT_`` and the count towards ``reference_update_frequency``. ``AppSession``
is that loop in frame-to-reference mode (aicp_hip_session_*): the reference, ``initialT_``, the count
and the last reading live in HBM, a reading crosses the bus at most once, and a reading that comes
from a ``SweepAccumulator`` does not cross it at all.

    acc.push(sweep, pose) ...                    # processLidar
    if motion_gate(prev_pose, pose):             # velodyneCallBack's test
        T, result, kept = session.process(acc, pose[:3, 3])
    acc.clear()

With ``risk=dict(model=SvmModel, threshold=..., params=RiskParams)`` the session serves
``failure_prediction_mode`` (aicp_hip_session_create_risk): every reading goes through the overlap,
the alignment features and the classifier on the resident buffers, and a reading whose risk is above
the threshold becomes the reference unmoved, on the device, instead of being registered. Such a
session takes 4x4 prior poses in place of origins:

    session.start(first, pose=first_pose)
    T, result, kept, record = session.process(reading, pose=prior_pose)

With ``keep_aligned_map=True`` the session also keeps App's ``aligned_map_`` (app.cpp:310, 458-468)
on the device: the first cloud's reference and every later reference, appended where the promotion
happens. ``aligned_map`` is a borrowed view of it, and the go-back of the node
(app_ros.cpp:329-357) moves no point over the bus:

    prior = session.take_aligned_map()           # the session's map, now the caller's PriorMap
    loc = MapSession(ctx, prior, params=L.default_localization_params())
    loc.start_go_back(session)                   # App's graph count and initialT_, device to device

``start_on_map(prior_map, pose)`` is ``load_map_from_file`` without localising (app.cpp:43-59,
392-399): the reference is the loaded map's crop around the first reading's prior pose.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .accumulator import SweepAccumulator


class AppSession(L.SessionMonitor):
    _monitor_kind = "session"

    def __init__(self, ctx: "L.Context", cfg=None, params=None, prefilter=None, risk=None, monitor=None,
                 keep_aligned_map=False):
        """cfg: IcpConfig (default_config() when None; a point-to-point chain is accepted); params:
        SequenceParams (flags: AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN); prefilter:
        None when the clouds are already pre-filtered, PrefilterParams (or True for the defaults)
        when they are RAW and go through setAndFilterReading in App's order; risk: None, or
        dict(model=SvmModel (kept alive by the session), threshold=float (default 0.5),
        params=RiskParams (default_risk_params() when left out)) for failure_prediction_mode;
        monitor: None (off), True or dict(quantile=, max_accepted_dist=, paired=) for the quality
        monitor per reading (set_monitor, last_monitor, monitor_counters); keep_aligned_map: keep
        App's aligned_map_ on the device from the next start on (aligned_map, take_aligned_map)."""
        mon = L.monitor_argument(monitor)  # (a bad argument before anything is made)
        cfg = cfg or L.default_config()
        prm = params or L.default_sequence_params()
        if prefilter is True:
            prefilter = L.default_prefilter()
        h = C.c_void_p()
        pf = None if prefilter is None else C.byref(prefilter)
        self.risk = None
        if risk is not None:
            unknown = set(risk) - {"model", "threshold", "params"}
            if unknown or "model" not in risk:
                raise ValueError(f"risk: dict(model=, threshold=, params=), got {sorted(risk)}")
            rp = risk.get("params") or L.default_risk_params()
            self.risk = dict(model=risk["model"], threshold=float(risk.get("threshold", 0.5)), params=rp)
            ctx.check(L.lib.aicp_hip_session_create_risk(ctx.h, C.byref(cfg), C.byref(prm), pf, C.byref(rp),
                                                         risk["model"].h, self.risk["threshold"], C.byref(h)))
        else:
            ctx.check(L.lib.aicp_hip_session_create(ctx.h, C.byref(cfg), C.byref(prm), pf, C.byref(h)))
        self.ctx = ctx
        self.h = h
        if mon is not None:
            self.set_monitor(mon)
        if keep_aligned_map:
            self.keep_aligned_map(True)

    def keep_aligned_map(self, on=True) -> None:
        """aicp_hip_session_keep_aligned_map: from the next start on (off: a map held is freed)."""
        self.ctx.check(L.lib.aicp_hip_session_keep_aligned_map(self.ctx.h, self.h, 1 if on else 0))

    @property
    def aligned_map(self):
        """App's aligned_map_ as a borrowed PriorMap view (len, getCloud, crop, capacity), valid
        until the next start, take_aligned_map or close. AicpError when keeping is off, the session
        has not started, or the map was taken."""
        from .prior_map import PriorMap

        h = C.c_void_p()
        self.ctx.check(L.lib.aicp_hip_session_aligned_map(self.ctx.h, self.h, C.byref(h)))
        return PriorMap.from_handle(self.ctx, h, owning=False)

    def take_aligned_map(self):
        """The aligned map as an owning PriorMap; nothing is copied. The session keeps running
        and no longer accumulates until its next start."""
        from .prior_map import PriorMap

        h = C.c_void_p()
        self.ctx.check(L.lib.aicp_hip_session_take_aligned_map(self.ctx.h, self.h, C.byref(h)))
        return PriorMap.from_handle(self.ctx, h, owning=True)

    def start_on_map(self, prior_map, pose, crop=15.0) -> None:
        """load_map_from_file without localising (app.cpp:43-59, 392-399): the reference is
        prior_map cropped to [-crop, crop]^3 around pose (the first reading's 4x4 prior pose); the
        first reading is registered against it without the drop test and becomes the next
        reference whatever the frequency. A plain session's call."""
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(4, 4).T.reshape(16))
        self.ctx.check(L.lib.aicp_hip_session_start_on_map(self.ctx.h, self.h, prior_map.h, L._fptr(p),
                                                           -float(crop), float(crop)))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                L.lib.aicp_hip_session_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _origin(origin):
        o = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(3))
        return o, L._dptr(o)

    def _pose(self, pose):
        """A risk session's pose argument (4x4 row-major) as column-major double[16]."""
        if self.risk is None:
            if pose is not None:
                raise TypeError("pose= is a risk session's argument (AppSession(..., risk=...))")
            return None
        if pose is None:
            raise TypeError("a risk session takes pose= (4x4 prior pose), not an origin")
        p = L._pose16(pose)
        return p, L._dptr(p)

    def start(self, first, origin=(0, 0, 0), pose=None) -> None:
        """The first cloud ((N, 3|4|8|12) float32 rows, or a SweepAccumulator) with its sensor
        origin (a risk session: pose=, its 4x4 pose): pre-filtered as given when the session has a
        pre-filter; it becomes reference -1. Calling it again restarts the session."""
        pp = self._pose(pose)
        if pp is not None:
            if isinstance(first, SweepAccumulator):
                self.ctx.check(L.lib.aicp_hip_session_start_accum_pose(self.ctx.h, self.h, first.h, pp[1]))
            else:
                c, keep = L.make_cloud(first, pp[0][12:15])
                self.ctx.check(L.lib.aicp_hip_session_start_pose(self.ctx.h, self.h, C.byref(c), pp[1]))
            return
        if isinstance(first, SweepAccumulator):
            o, op = self._origin(origin)
            self.ctx.check(L.lib.aicp_hip_session_start_accum(self.ctx.h, self.h, first.h, op))
            return
        c, keep = L.make_cloud(first, origin)
        self.ctx.check(L.lib.aicp_hip_session_start(self.ctx.h, self.h, C.byref(c)))

    def process(self, reading, origin=(0, 0, 0), raise_on_error=True, pose=None):
        """One reading (rows, or a SweepAccumulator, which is left as it is) with its prior-pose
        origin. Returns (T 4x4 row-major correction, result dict as Context.sequence_run's with `rc`
        added, kept points). A failed reading ends the session (AicpError unless raise_on_error is
        False); start() revives it. A risk session takes pose= (the 4x4 prior pose) and returns the
        pipeline's record dict (Context.pipeline's) as a fourth value."""
        outT = np.zeros(16, np.float32)
        res = L.SequenceResult()
        kept = C.c_uint32(0)
        pp = self._pose(pose)
        if pp is not None:
            rec = L.PipelineRecord()
            if isinstance(reading, SweepAccumulator):
                rc = L.lib.aicp_hip_session_process_accum_risk(self.ctx.h, self.h, reading.h, pp[1], L._fptr(outT),
                                                               C.byref(res), C.byref(rec), C.byref(kept))
            else:
                c, keep = L.make_cloud(reading, pp[0][12:15])
                rc = L.lib.aicp_hip_session_process_risk(self.ctx.h, self.h, C.byref(c), pp[1], L._fptr(outT),
                                                         C.byref(res), C.byref(rec), C.byref(kept))
            if raise_on_error and rc != L.AICP_OK:
                self.ctx.check(rc)
            d = res.as_dict()
            d["rc"] = rc
            return outT.reshape(4, 4).T.copy(), d, int(kept.value), rec.as_dict()
        if isinstance(reading, SweepAccumulator):
            o, op = self._origin(origin)
            rc = L.lib.aicp_hip_session_process_accum(self.ctx.h, self.h, reading.h, op, L._fptr(outT), C.byref(res),
                                                      C.byref(kept))
        else:
            c, keep = L.make_cloud(reading, origin)
            rc = L.lib.aicp_hip_session_process(self.ctx.h, self.h, C.byref(c), L._fptr(outT), C.byref(res),
                                                C.byref(kept))
        if raise_on_error and rc != L.AICP_OK:
            self.ctx.check(rc)
        d = res.as_dict()
        d["rc"] = rc
        return outT.reshape(4, 4).T.copy(), d, int(kept.value)

    def state(self) -> dict:
        """n_processed (process calls since start), reference (-1: the first cloud, else the index
        of the process call whose reading it is), reference_points, initial_T (4x4 row-major),
        ended."""
        n, ref, pts, ended = C.c_uint64(), C.c_int32(), C.c_size_t(), C.c_int32()
        T = np.zeros(16, np.float32)
        self.ctx.check(L.lib.aicp_hip_session_state(self.ctx.h, self.h, C.byref(n), C.byref(ref), C.byref(pts),
                                                    L._fptr(T), C.byref(ended)))
        return dict(n_processed=int(n.value), reference=int(ref.value), reference_points=int(pts.value),
                    initial_T=T.reshape(4, 4).T.copy(), ended=bool(ended.value))

    def reference(self):
        """The current reference (App's reference_vis_): ((N, 3) float32 points, origin (3,) float64)."""
        n = self.state()["reference_points"]
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_size_t()
        o = np.zeros(3, np.float64)
        self.ctx.check(L.lib.aicp_hip_session_reference(self.ctx.h, self.h, L._fptr(out), n, C.byref(m), L._dptr(o)))
        return out[:m.value].copy(), o

    def reference_pose(self):
        """A risk session's current reference pose (4x4 row-major float64): App's corrected pose of
        the reading that became the reference, through removePitchRollCorrection."""
        p = np.zeros(16, np.float64)
        self.ctx.check(L.lib.aicp_hip_session_reference_pose(self.ctx.h, self.h, L._dptr(p)))
        return p.reshape(4, 4).T.copy()

    def last_timing(self) -> dict:
        """wall_ms / device_ms of the last process call that registered its reading."""
        w, d = C.c_double(), C.c_double()
        self.ctx.check(L.lib.aicp_hip_session_last_timing(self.h, C.byref(w), C.byref(d)))
        return dict(wall_ms=w.value, device_ms=d.value)
