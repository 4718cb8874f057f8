"""Device-resident sweep accumulator: how a raw reading comes to exist.

The reference assembles a reading in ``VelodyneAccumulatorROS::processLidar``
(aicp_ros/src/velodyne_accumulator.cpp:31-73), driven by ``AppROS::velodyneCallBack``
(aicp_ros/src/app_ros.cpp:178-256): every lidar sweep is cropped to +-30 m around the sensor, moved
into the inertial frame by the sweep's pose and appended, until ``batch_size`` sweeps are in; the
cloud is handed on only if the robot moved more than 1 m or 10 degrees since the last one.

``SweepAccumulator`` does the same in HBM (aicp_hip_accum_*): a sweep is uploaded when it is pushed
and cropped, moved and appended on the device, so the raw reading never exists on the host.
``prefilter`` runs the pre-filter on it where it lies and returns the kept points, which every
existing entry point takes as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def pose_matrix(pose) -> np.ndarray:
    """aicp_hip_accum_pose_matrix: the float 4x4 (row-major) by which a sweep with the Isometry3d
    `pose` (4x4 row-major, inertial <- sensor) is moved (velodyne_accumulator.cpp:62-63). Host only."""
    out = np.zeros(16, np.float32)
    L.lib.aicp_hip_accum_pose_matrix(L._dptr(L._pose16(pose)), L._fptr(out))
    return out.reshape(4, 4).T.copy()


def motion_gate(prev, pose, min_dist: float = 1.0, min_angle_rad: float = 10.0 * np.pi / 180.0) -> bool:
    """aicp_hip_motion_gate (app_ros.cpp:203-213): did the robot move more than min_dist, or turn
    more than min_angle_rad about any axis, between the 4x4 row-major poses prev and pose? Host only."""
    return bool(L.lib.aicp_hip_motion_gate(L._dptr(L._pose16(prev)), L._dptr(L._pose16(pose)), float(min_dist),
                                           float(min_angle_rad)))


def default_accum_params(**kw) -> "L.AccumParams":
    """aicp_hip_default_accum_params (batch_size 80, crop -30 .. 30) with keyword overrides."""
    p = L.AccumParams()
    L.lib.aicp_hip_default_accum_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"aicp_accum_params has no field {k}")
        setattr(p, k, v)
    return p


class SweepAccumulator:
    def __init__(self, ctx: "L.Context", capacity_points: int, params=None, **kw):
        """capacity_points: the most input points one reading's sweeps may add up to; params:
        AccumParams (default_accum_params(**kw) when None)."""
        prm = params or default_accum_params(**kw)
        h = C.c_void_p()
        ctx.check(L.lib.aicp_hip_accum_create(ctx.h, C.byref(prm), int(capacity_points), C.byref(h)))
        self.ctx = ctx
        self.h = h
        self.batch_size = int(prm.batch_size)
        self.capacity = int(capacity_points)

    def free(self):
        if getattr(self, "h", None):
            L.lib.aicp_hip_accum_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        self.free()

    def push(self, points, pose) -> None:
        """processLidar for one sweep ((N, 3|4|8|12) float32 rows, N may be 0; pose: 4x4 row-major
        Isometry3d). Does not wait for the device; `points` is free to be rewritten on return. A
        sweep that does not fit the capacity raises AicpError (AICP_ERR_INVALID) and changes nothing."""
        pts = L.as_points(points)
        self.ctx.check(L.lib.aicp_hip_accum_push(self.ctx.h, self.h, L._fptr(pts), pts.shape[0], pts.shape[1] * 4,
                                                 L._dptr(L._pose16(pose))))

    def _state(self, kept=None):
        c, f, n = C.c_int32(), C.c_int32(), C.c_size_t()
        self.ctx.check(L.lib.aicp_hip_accum_state(
            self.ctx.h, self.h, C.byref(c), C.byref(f), C.byref(n),
            None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_uint32))))
        return c.value, bool(f.value), n.value

    @property
    def counter(self) -> int:
        """getCounter(): sweeps taken since the last clear."""
        return self._state()[0]

    @property
    def finished(self) -> bool:
        """getFinished(): batch_size sweeps are in; further pushes are ignored."""
        return self._state()[1]

    def __len__(self):
        """Points accumulated so far (waits for the pushes enqueued so far)."""
        return self._state()[2]

    def kept_per_sweep(self) -> np.ndarray:
        """(batch_size,) uint32: the points each sweep kept after the crop (0 for sweeps not taken)."""
        kept = np.zeros(self.batch_size, np.uint32)
        self._state(kept)
        return kept

    def getCloud(self) -> np.ndarray:
        """The accumulated cloud (VelodyneAccumulatorROS::getCloud), (N, 3) float32."""
        n = len(self)
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_size_t()
        self.ctx.check(L.lib.aicp_hip_accum_download(self.ctx.h, self.h, L._fptr(out), n, C.byref(m)))
        return out[:m.value].copy()

    def clear(self) -> None:
        """clearCloud()."""
        self.ctx.check(L.lib.aicp_hip_accum_clear(self.ctx.h, self.h))

    def prefilter(self, T=None, params=None) -> np.ndarray:
        """regionGrowingUniformPlaneSegmentationFilter of the accumulated cloud on the device
        (aicp_hip_accum_prefilter), moved first by the 4x4 row-major T when it is given (App's debug
        working mode, app.cpp:87-99). Returns the kept points, (M, 3) float32; the accumulator keeps
        its cloud."""
        prm = params or L.default_prefilter()
        t = None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T.reshape(16))
        n = len(self)
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_size_t()
        self.ctx.check(L.lib.aicp_hip_accum_prefilter(self.ctx.h, self.h, C.byref(prm),
                                                      None if t is None else L._fptr(t), L._fptr(out), n, C.byref(m)))
        return out[:m.value].copy()
