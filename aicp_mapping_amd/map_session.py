"""Live map sessions: App::processCloud on the prior map or on the built map, one reading per call.

``PriorMap.sequence_run`` / ``BuiltMap.sequence_run`` take a whole recording. A node receives its
readings one by one: ``MapSession`` (aicp_hip_map_session_*) handles one per call against the
device-resident map and keeps App's state for the policy, ``initialT_`` and the count, on the
device between calls. Reading by reading the rules are the streams'; the append to the map is
decided and done on the device behind the reading's registration.

    session = MapSession(ctx, prior_map, params=L.default_localization_params(), prefilter=True)
    session.start()
    for reading, pose in node:                   # or a SweepAccumulator in place of the reading
        T, result, kept = session.process(reading, pose)

With ``risk=dict(model=SvmModel, threshold=..., params=RiskParams)`` the session serves
``failure_prediction_mode`` under the map's policy (aicp_hip_mapsession_create_risk): every reading
goes through the overlap (built map; the prior map's is the constant 50), the alignment features and
the classifier on the crop and the reading where they lie on the device, and a reading whose risk is
above the threshold is not registered: on the built map it becomes the reference unmoved, on the
prior map it joins the graph without a merge. ``process`` then takes the 4x4 prior pose in double
and returns the pipeline's record as a fourth value:

    T, result, kept, record = session.process(reading, pose)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .accumulator import SweepAccumulator
from .built_map import BuiltMap


class MapSession(L.SessionMonitor):
    _monitor_kind = "mapsession"

    def __init__(self, ctx: "L.Context", map, cfg=None, params=None, prefilter=None, map_prefilter=None,
                 monitor=None, risk=None):
        """map: a PriorMap (localize_against_prior_map; params: LocalizationParams) or a BuiltMap
        (localize_against_built_map, created from App's first cloud; params: BuiltMapParams); the
        policy follows the map's class and the params' type, which must agree. cfg: IcpConfig
        (default_config() when None; a point-to-point chain is accepted). prefilter: None when the
        readings are already pre-filtered, PrefilterParams (or True for the defaults) when they
        are RAW and go through setAndFilterReading in App's order. map_prefilter: the prior map's
        re-filter (None: the defaults); not for a BuiltMap. monitor: None (off), True or
        dict(quantile=, max_accepted_dist=, paired=) for the quality monitor per reading, against
        the reading's map crop (set_monitor, last_monitor, monitor_counters). risk: None, or
        dict(model=SvmModel (kept alive by the session), threshold=float (default 0.5),
        params=RiskParams (default_risk_params() when left out)) for failure_prediction_mode; on a
        BuiltMap the overlap then always runs."""
        mon = L.monitor_argument(monitor)  # (a bad argument before anything is made)
        built = isinstance(map, BuiltMap)
        if params is None:
            params = L.default_built_map_params() if built else L.default_localization_params()
        if isinstance(params, L.BuiltMapParams) != built:
            raise TypeError("MapSession: a BuiltMap takes BuiltMapParams, a PriorMap LocalizationParams")
        cfg = cfg or L.default_config()
        if prefilter is True:
            prefilter = L.default_prefilter()
        h = C.c_void_p()
        args = (ctx.h, C.byref(cfg), None if built else C.byref(params), C.byref(params) if built else None,
                None if prefilter is None else C.byref(prefilter),
                None if map_prefilter is None else C.byref(map_prefilter))
        self.risk = None
        if risk is not None:
            unknown = set(risk) - {"model", "threshold", "params"}
            if unknown or "model" not in risk:
                raise ValueError(f"risk: dict(model=, threshold=, params=), got {sorted(risk)}")
            rp = risk.get("params") or L.default_risk_params()
            self.risk = dict(model=risk["model"], threshold=float(risk.get("threshold", 0.5)), params=rp)
            ctx.check(L.lib.aicp_hip_mapsession_create_risk(*args, C.byref(rp), risk["model"].h,
                                                            self.risk["threshold"], C.byref(h)))
        else:
            ctx.check(L.lib.aicp_hip_map_session_create(*args, C.byref(h)))
        self.ctx = ctx
        self.map = map
        self.built = built
        self.h = h
        if mon is not None:
            self.set_monitor(mon)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                L.lib.aicp_hip_map_session_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        self.close()

    def start(self) -> None:
        """count = 0, initialT_ = I, not ended. Calling it again restarts the session on the map
        as it is now."""
        self.ctx.check(L.lib.aicp_hip_map_session_start(self.ctx.h, self.h, self.map.h))

    def start_go_back(self, app_session) -> None:
        """The node's go-back (app_ros.cpp:329-357) for a session on a PriorMap: start() with App's
        state in place of a fresh one, the count at app_session's graph size (its first cloud and
        its accepted readings) and its initialT_, copied device to device. The map is usually
        app_session.take_aligned_map()."""
        self.ctx.check(L.lib.aicp_hip_mapsession_start_go_back(self.ctx.h, self.h, self.map.h, app_session.h))

    def process(self, reading, pose, raise_on_error=True):
        """One reading ((N, 3|4|8|12) float32 rows, or a SweepAccumulator, which is left as it is)
        with its 4x4 row-major prior pose, whose translation is the reading's sensor origin.
        Returns (T 4x4 row-major correction, result dict as the map's sequence_run gives them with
        `rc` added, kept points). An empty crop, an emptied reading or a registration error ends
        the session (AicpError unless raise_on_error is False); start() revives it. A risk session
        reads the pose in double (the crop is taken at its float cast), ends on a failed overlap,
        feature or classifier step too, and returns the pipeline's record dict (Context.pipeline's)
        as a fourth value."""
        if self.risk is not None:
            return self._process_risk(reading, pose, raise_on_error)
        P = np.asarray(pose, np.float64).reshape(4, 4)
        pz = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(4, 4).T.reshape(16))
        outT = np.zeros(16, np.float32)
        res = (L.BuiltMapResult if self.built else L.LocalizationResult)()
        kept = C.c_uint32(0)
        if isinstance(reading, SweepAccumulator):
            rc = L.lib.aicp_hip_map_session_process_accum(self.ctx.h, self.h, reading.h, L._fptr(pz), L._fptr(outT),
                                                          C.byref(res), C.byref(kept))
        else:
            c, keep = L.make_cloud(reading, P[:3, 3])
            rc = L.lib.aicp_hip_map_session_process(self.ctx.h, self.h, C.byref(c), L._fptr(pz), L._fptr(outT),
                                                    C.byref(res), C.byref(kept))
        if raise_on_error and rc != L.AICP_OK:
            self.ctx.check(rc)
        d = res.as_dict()
        d["rc"] = rc
        return outT.reshape(4, 4).T.copy(), d, int(kept.value)

    def _process_risk(self, reading, pose, raise_on_error):
        pd = L._pose16(pose)
        outT = np.zeros(16, np.float32)
        res = (L.BuiltMapResult if self.built else L.LocalizationResult)()
        kept = C.c_uint32(0)
        rec = L.PipelineRecord()
        if isinstance(reading, SweepAccumulator):
            rc = L.lib.aicp_hip_mapsession_process_accum_risk(self.ctx.h, self.h, reading.h, L._dptr(pd), L._fptr(outT),
                                                              C.byref(res), C.byref(rec), C.byref(kept))
        else:
            c, keep = L.make_cloud(reading, pd[12:15])
            rc = L.lib.aicp_hip_mapsession_process_risk(self.ctx.h, self.h, C.byref(c), L._dptr(pd), L._fptr(outT),
                                                        C.byref(res), C.byref(rec), C.byref(kept))
        if raise_on_error and rc != L.AICP_OK:
            self.ctx.check(rc)
        d = res.as_dict()
        d["rc"] = rc
        return outT.reshape(4, 4).T.copy(), d, int(kept.value), rec.as_dict()

    def state(self) -> dict:
        """n_processed (process calls since start), count (prior map: the accepted readings; built
        map: those since the last reference), initial_T (4x4 row-major), ended."""
        n, cnt, ended = C.c_uint64(), C.c_int32(), C.c_int32()
        T = np.zeros(16, np.float32)
        self.ctx.check(L.lib.aicp_hip_map_session_state(self.ctx.h, self.h, C.byref(n), C.byref(cnt), L._fptr(T),
                                                        C.byref(ended)))
        return dict(n_processed=int(n.value), count=int(cnt.value), initial_T=T.reshape(4, 4).T.copy(),
                    ended=bool(ended.value))

    def last_timing(self) -> dict:
        """wall_ms / device_ms of the last process call that registered its reading (a risk
        session: or gated it)."""
        w, d = C.c_double(), C.c_double()
        self.ctx.check(L.lib.aicp_hip_map_session_last_timing(self.h, C.byref(w), C.byref(d)))
        return dict(wall_ms=w.value, device_ms=d.value)
