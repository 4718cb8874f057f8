"""App's localization against the map it has built itself (localize_against_built_map).

In this reference policy (setReference, app.cpp:60-69) every reading is registered against
``aligned_map_``, the map App builds from its own aligned clouds, cropped around the reading's
prior pose. Unlike localization against a prior map the octree overlap is not bypassed
(app.cpp:123-135): every reading gets the overlap against its own crop and the auto-tuned ratio
from it. The map starts as the first cloud (app.cpp:293-310), grows by every
``reference_update_frequency``-th accepted reading (app.cpp:383-391, 458-465) and is never
re-filtered.

``BuiltMap`` is a ``PriorMap`` (the same device-resident cloud and handle: crop, merge, getCloud,
free) with the batch entry that keeps the overlap (aicp_hip_map_align_batch) and the stream
(aicp_hip_built_map_sequence_run).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .prior_map import PriorMap, _clouds_and_poses, _stream_results


class BuiltMap(PriorMap):
    def __init__(self, ctx: "L.Context", first_cloud):
        """first_cloud: App's first cloud, already pre-filtered (aligned_map_ = first cloud)."""
        super().__init__(ctx, first_cloud)

    def align_batch(self, readings, poses, mn: float = -15.0, mx: float = 15.0, cfg=None, resolution: float = 0.2,
                    flags: int = L.AICP_RUN_OVERLAP, raise_on_error=True):
        """aicp_hip_map_align_batch: reading i against this map cropped on the device around poses[i]
        (4x4 row-major prior pose; its translation is the reading's sensor origin and the crop's).
        flags: AICP_RUN_OVERLAP (the octree overlap of each pair and the auto-tuned ratio from it;
        without it cfg.trimmed_ratio) | AICP_RUN_TIME_NN. Returns (T[n, 4, 4] row-major, list of
        stats dicts, rc)."""
        cfg = cfg or L.default_config()
        n = len(readings)
        arr, pz, keep = _clouds_and_poses(readings, poses)
        outT = np.zeros((max(n, 1), 16), np.float32)
        st = (L.IcpStats * max(n, 1))()
        rc = L.lib.aicp_hip_map_align_batch(self.ctx.h, C.byref(cfg), self.h, float(mn), float(mx), arr, L._fptr(pz), n,
                                            float(resolution), int(flags), L._fptr(outT), st)
        if raise_on_error and rc != L.AICP_OK:
            self.ctx.check(rc)
        return outT[:n].reshape(-1, 4, 4).transpose(0, 2, 1).copy(), [st[i].as_dict() for i in range(n)], rc

    def sequence_run(self, readings, poses, cfg=None, params=None, raise_on_error=True, raw=False,
                     read_prefilter=None):
        """App's stream in this mode (aicp_hip_built_map_sequence_run): reading i is registered
        against the map cropped around poses[i] with its own overlap and ratio, dropped on a large
        correction (the first reading too), and every reference_update_frequency-th accepted
        reading is appended to the map, in place. params: BuiltMapParams
        (default_built_map_params). Returns (T[n, 4, 4] row-major corrections, list of result dicts
        of the readings processed, n_done, rc); a registration error ends the stream at reading
        n_done - 1 and raises unless raise_on_error is False.
        raw=True (aicp_hip_built_map_sequence_run_raw): the readings are RAW clouds, pre-filtered
        inside the stream in App's order (debug mode: moved by initialT_ first) with read_prefilter
        (PrefilterParams; None: the defaults); the return value gains a fifth element, the (n,)
        uint32 counts of the points each reading kept."""
        cfg = cfg or L.default_config()
        prm = params or L.default_built_map_params()
        n = len(readings)
        arr, pz, keep = _clouds_and_poses(readings, poses)
        outT = np.zeros((max(n, 1), 16), np.float32)
        res = (L.BuiltMapResult * max(n, 1))()
        done = C.c_size_t(0)
        if not raw:
            rc = L.lib.aicp_hip_built_map_sequence_run(self.ctx.h, C.byref(cfg), C.byref(prm), self.h, arr, L._fptr(pz),
                                                       n, L._fptr(outT), res, C.byref(done))
            return _stream_results(self.ctx, rc, raise_on_error, n, outT, res, done)
        pfr = read_prefilter if read_prefilter is not None else L.default_prefilter()
        kept = np.zeros(max(n, 1), np.uint32)
        rc = L.lib.aicp_hip_built_map_sequence_run_raw(self.ctx.h, C.byref(cfg), C.byref(prm), C.byref(pfr), self.h, arr,
                                                       L._fptr(pz), n, L._fptr(outT), res,
                                                       kept.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(done))
        return _stream_results(self.ctx, rc, raise_on_error, n, outT, res, done) + (kept[:n],)
