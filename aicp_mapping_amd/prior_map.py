"""Device-resident prior map of aicp_core's localization mode.

App keeps ``prior_map_`` (an AlignedCloud) and, in localization mode:
- crops it around each reading's prior pose to make the reference (``setReference``,
  app.cpp:41-51, ``getPointsInOrientedBox`` filteringUtils.cpp:619-637);
- appends the aligned reading every ``reference_update_frequency`` clouds when
  ``merge_aligned_clouds_to_map`` (app.cpp:469-483: ``*merged_map = *prior_map + *output`` with
  ``output = transformPointCloud(read_prefiltered, correction)``);
- pre-filters the whole map every 30 clouds (app.cpp:485-493).

``PriorMap`` holds the map in HBM (aicp_hip_map_*) so none of these steps re-uploads it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _clouds_and_poses(readings, poses):
    """The aicp_cloud array (origin: the prior pose's translation) and the column-major poses of a
    batch or stream call (at least one slot each), and the arrays the clouds point into."""
    n = len(readings)
    arr = (L.Cloud * max(n, 1))()
    keep = []
    pz = np.zeros((max(n, 1), 16), np.float32)
    for i, r in enumerate(readings):
        P = np.asarray(poses[i], np.float64).reshape(4, 4)
        c, k = L.make_cloud(r, P[:3, 3])
        arr[i] = c
        keep.append(k)
        pz[i] = np.asarray(poses[i], np.float32).reshape(4, 4).T.reshape(16)
    return arr, pz, keep


def _stream_results(ctx, rc, raise_on_error, n, outT, res, done):
    """The shared tail of the two sequence_run wrappers: (T, result dicts, n_done, rc)."""
    if raise_on_error and rc != L.AICP_OK:
        ctx.check(rc)
    T = outT[:n].reshape(-1, 4, 4).transpose(0, 2, 1).copy()
    return T, [res[i].as_dict() for i in range(done.value)], done.value, rc


class PriorMap:
    def __init__(self, ctx: "L.Context", points):
        pts = L.as_points(points)
        h = C.c_void_p()
        ctx.check(L.lib.aicp_hip_map_create(ctx.h, L._fptr(pts), pts.shape[0], pts.shape[1] * 4, C.byref(h)))
        self.ctx = ctx
        self.h = h

    @classmethod
    def from_handle(cls, ctx: "L.Context", h, owning: bool = True) -> "PriorMap":
        """A PriorMap over an aicp_hip_map that already lies on the device (a live session's
        aligned map). owning=False: a borrowed view, which never frees the handle and is valid
        only as long as its owner keeps the map."""
        m = cls.__new__(cls)
        m.ctx = ctx
        m.h = h
        m.borrowed = not owning
        return m

    def free(self):
        if getattr(self, "h", None):
            if not getattr(self, "borrowed", False) and getattr(self.ctx, "h", None):
                L.lib.aicp_hip_map_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        self.free()

    def __len__(self):
        n = C.c_size_t()
        L.lib.aicp_hip_map_size(self.h, C.byref(n))
        return n.value

    @property
    def capacity(self) -> int:
        """Points the map's buffer holds before the next append has to grow it (aicp_hip_map_capacity)."""
        n = C.c_size_t()
        L.lib.aicp_hip_map_capacity(self.h, C.byref(n))
        return n.value

    def getCloud(self) -> np.ndarray:
        """The map's points (AlignedCloud::getCloud), (N, 3) float32."""
        n = len(self)
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_size_t()
        self.ctx.check(L.lib.aicp_hip_map_download(self.ctx.h, self.h, L._fptr(out), n, C.byref(m)))
        return out[:m.value].copy()

    def crop(self, mn: float, mx: float, origin) -> np.ndarray:
        """getPointsInOrientedBox(map, mn, mx, origin) on device; origin a 4x4 pose (row-major)."""
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(4, 4).T.reshape(16))
        n = len(self)
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_size_t()
        self.ctx.check(L.lib.aicp_hip_map_crop(self.ctx.h, self.h, float(mn), float(mx), L._fptr(o), L._fptr(out),
                                               n, C.byref(m)))
        return out[:m.value].copy()

    def register_batch(self, readings, poses, mn: float = -15.0, mx: float = 15.0, cfg=None, flags: int = 0):
        """Localization-only registration of a batch (aicp_hip_map_register_batch): reading i
        against this map cropped on the device around poses[i] (4x4 row-major prior pose), overlap
        fixed at 50 % (app.cpp:41-51,123-127). readings: list of (N, 3|4|8|12) float32 rows.
        Returns (T[n, 4, 4] row-major, list of stats dicts, rc)."""
        cfg = cfg or L.default_config()
        n = len(readings)
        arr, pz, keep = _clouds_and_poses(readings, poses)
        outT = np.zeros((n, 16), np.float32)
        st = (L.IcpStats * n)()
        rc = L.lib.aicp_hip_map_register_batch(self.ctx.h, C.byref(cfg), self.h, float(mn), float(mx), arr, L._fptr(pz),
                                               n, int(flags), L._fptr(outT), st)
        if rc != L.AICP_OK:
            self.ctx.check(rc)
        return outT.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), [x.as_dict() for x in st], rc

    def sequence_run(self, readings, poses, cfg=None, params=None, prefilter=None, raise_on_error=True, raw=False,
                     read_prefilter=None):
        """App's localization stream on this map (aicp_hip_map_sequence_run, app.cpp:282-414 with
        app.cpp:41-58, 469-493): reading i is registered against the map cropped around poses[i]
        (4x4 row-major prior pose; its translation is the reading's origin), dropped on a large
        correction, merged into the map every reference_update_frequency-th accepted reading, and
        the map re-filtered every map_refilter_every-th; the map is updated in place. params:
        LocalizationParams (default_localization_params); prefilter: the re-filter's
        PrefilterParams (None: the defaults). Returns (T[n, 4, 4] row-major corrections, list of
        result dicts of the readings processed, n_done, rc); a registration error ends the stream
        at reading n_done - 1 and raises unless raise_on_error is False.
        raw=True (aicp_hip_map_sequence_run_raw): the readings are RAW clouds, pre-filtered inside
        the stream in App's order (debug mode: moved by initialT_ first) with read_prefilter
        (PrefilterParams; None: the defaults); the return value gains a fifth element, the (n,)
        uint32 counts of the points each reading kept."""
        cfg = cfg or L.default_config()
        prm = params or L.default_localization_params()
        n = len(readings)
        arr, pz, keep = _clouds_and_poses(readings, poses)
        outT = np.zeros((max(n, 1), 16), np.float32)
        res = (L.LocalizationResult * max(n, 1))()
        done = C.c_size_t(0)
        pf_map = C.byref(prefilter) if prefilter is not None else None
        if not raw:
            rc = L.lib.aicp_hip_map_sequence_run(self.ctx.h, C.byref(cfg), C.byref(prm), pf_map, self.h, arr,
                                                 L._fptr(pz), n, L._fptr(outT), res, C.byref(done))
            return _stream_results(self.ctx, rc, raise_on_error, n, outT, res, done)
        pfr = read_prefilter if read_prefilter is not None else L.default_prefilter()
        kept = np.zeros(max(n, 1), np.uint32)
        rc = L.lib.aicp_hip_map_sequence_run_raw(self.ctx.h, C.byref(cfg), C.byref(prm), pf_map, C.byref(pfr), self.h,
                                                 arr, L._fptr(pz), n, L._fptr(outT), res,
                                                 kept.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(done))
        return _stream_results(self.ctx, rc, raise_on_error, n, outT, res, done) + (kept[:n],)

    def merge(self, points, correction) -> None:
        """*map = *map + transformPointCloud(points, correction); correction a 4x4 (row-major)."""
        pts = L.as_points(points)
        t = np.ascontiguousarray(np.asarray(correction, np.float32).reshape(4, 4).T.reshape(16))
        self.ctx.check(L.lib.aicp_hip_map_merge(self.ctx.h, self.h, L._fptr(pts), pts.shape[0], pts.shape[1] * 4,
                                                L._fptr(t)))

    def prefilter(self, params=None) -> None:
        """map = regionGrowingUniformPlaneSegmentationFilter(map) on device."""
        prm = params or L.default_prefilter()
        self.ctx.check(L.lib.aicp_hip_map_prefilter(self.ctx.h, self.h, C.byref(prm)))


def load_map_from_file(ctx: "L.Context", path: str, prefilter=None) -> PriorMap:
    """The node's map loading (app_ros.cpp:301-315): the PLY file's points
    (cloud_io.load_ply_xyz, pcl::io::loadPLYFile<PointXYZ>) as a device-resident map, pre-filtered
    once with `prefilter` (PrefilterParams; None: the defaults) as the node pre-filters the loaded
    map before it hands it to App."""
    from .cloud_io import load_ply_xyz

    m = PriorMap(ctx, load_ply_xyz(path))
    m.prefilter(prefilter)
    return m


def localization_update(prior_map: PriorMap, read_prefiltered, correction, n_clouds: int,
                        reference_update_frequency: int = 5, merge_aligned_clouds_to_map: bool = True,
                        is_reference: bool = False) -> None:
    """App's map maintenance after an accepted alignment in localization mode (app.cpp:469-493);
    n_clouds = aligned_clouds_graph_->getNbClouds() after adding the reading."""
    if not is_reference and (n_clouds - 1) % reference_update_frequency == 0 and merge_aligned_clouds_to_map:
        prior_map.merge(read_prefiltered, correction)
    if merge_aligned_clouds_to_map and (n_clouds - 1) % 30 == 0:
        prior_map.prefilter()
