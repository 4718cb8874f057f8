"""aicp_mapping_amd — MI355X-native ICP registration core for AICP (zbqq/aicp_mapping).

The product is libaicp_hip.so (C-ABI in include/aicp_hip.h, HIP kernels for gfx950 under
csrc/). This package mirrors the reference's registrator / overlapper plugin interfaces on top
of it (registration.py), assembles raw readings from lidar sweeps on the device (accumulator.py:
SweepAccumulator, pose_matrix, motion_gate), runs App's loop one reading per call with its state on
the device (session.py: AppSession; map_session.py: MapSession, the two map policies) and ships the seeded synthetic scenes of the benchmark
(synthetic.py).
Importing `aicp_mapping_amd.registration` or `aicp_mapping_amd._lib` loads the HIP library and
fails loudly if it is missing.
"""

__all__ = ["registration", "synthetic", "accumulator", "session", "SweepAccumulator", "pose_matrix", "motion_gate",
           "AppSession", "map_session", "MapSession"]


def __getattr__(name):
    import importlib

    if name in ("registration", "_lib", "synthetic", "accumulator", "session", "map_session"):
        return importlib.import_module(f"{__name__}.{name}")
    if name in ("SweepAccumulator", "pose_matrix", "motion_gate"):
        return getattr(importlib.import_module(f"{__name__}.accumulator"), name)
    if name == "AppSession":
        return getattr(importlib.import_module(f"{__name__}.session"), name)
    if name == "MapSession":
        return getattr(importlib.import_module(f"{__name__}.map_session"), name)
    raise AttributeError(name)
