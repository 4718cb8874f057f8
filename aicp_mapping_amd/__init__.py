"""aicp_mapping_amd — MI355X-native ICP registration core for AICP (zbqq/aicp_mapping).

The product is libaicp_hip.so (C-ABI in include/aicp_hip.h, HIP kernels for gfx950 under
csrc/). This package mirrors the reference's registrator / overlapper plugin interfaces on top
of it (registration.py), assembles raw readings from lidar sweeps on the device (accumulator.py:
SweepAccumulator, pose_matrix, motion_gate) and ships the seeded synthetic scenes of the benchmark
(synthetic.py).
Importing `aicp_mapping_amd.registration` or `aicp_mapping_amd._lib` loads the HIP library and
fails loudly if it is missing.
"""

__all__ = ["registration", "synthetic", "accumulator", "SweepAccumulator", "pose_matrix", "motion_gate"]


def __getattr__(name):
    import importlib

    if name in ("registration", "_lib", "synthetic", "accumulator"):
        return importlib.import_module(f"{__name__}.{name}")
    if name in ("SweepAccumulator", "pose_matrix", "motion_gate"):
        return getattr(importlib.import_module(f"{__name__}.accumulator"), name)
    raise AttributeError(name)
