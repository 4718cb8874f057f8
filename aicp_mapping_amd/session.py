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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .accumulator import SweepAccumulator


class AppSession:
    def __init__(self, ctx: "L.Context", cfg=None, params=None, prefilter=None):
        """cfg: IcpConfig (default_config() when None; a point-to-point chain is accepted); params:
        SequenceParams (flags: AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN); prefilter:
        None when the clouds are already pre-filtered, PrefilterParams (or True for the defaults)
        when they are RAW and go through setAndFilterReading in App's order."""
        cfg = cfg or L.default_config()
        prm = params or L.default_sequence_params()
        if prefilter is True:
            prefilter = L.default_prefilter()
        h = C.c_void_p()
        ctx.check(L.lib.aicp_hip_session_create(ctx.h, C.byref(cfg), C.byref(prm),
                                                None if prefilter is None else C.byref(prefilter), C.byref(h)))
        self.ctx = ctx
        self.h = h

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

    def start(self, first, origin=(0, 0, 0)) -> None:
        """The first cloud ((N, 3|4|8|12) float32 rows, or a SweepAccumulator) with its sensor
        origin: pre-filtered as given when the session has a pre-filter; it becomes reference -1.
        Calling it again restarts the session."""
        if isinstance(first, SweepAccumulator):
            o, op = self._origin(origin)
            self.ctx.check(L.lib.aicp_hip_session_start_accum(self.ctx.h, self.h, first.h, op))
            return
        c, keep = L.make_cloud(first, origin)
        self.ctx.check(L.lib.aicp_hip_session_start(self.ctx.h, self.h, C.byref(c)))

    def process(self, reading, origin=(0, 0, 0), raise_on_error=True):
        """One reading (rows, or a SweepAccumulator, which is left as it is) with its prior-pose
        origin. Returns (T 4x4 row-major correction, result dict as Context.sequence_run's with `rc`
        added, kept points). A failed reading ends the session (AicpError unless raise_on_error is
        False); start() revives it."""
        outT = np.zeros(16, np.float32)
        res = L.SequenceResult()
        kept = C.c_uint32(0)
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

    def last_timing(self) -> dict:
        """wall_ms / device_ms of the last process call that registered its reading."""
        w, d = C.c_double(), C.c_double()
        self.ctx.check(L.lib.aicp_hip_session_last_timing(self.h, C.byref(w), C.byref(d)))
        return dict(wall_ms=w.value, device_ms=d.value)
