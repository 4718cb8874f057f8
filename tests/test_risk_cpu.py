"""Alignment-risk entry points without a device: exports, argument checks, defaults and the C++
shim header (integration/hip_alignability.hpp) against the stand-in PCL / Eigen types."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM = os.path.join(HERE, "shim")
LIB = os.path.join(ROOT, "aicp_mapping_amd", "libaicp_hip.so")


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


def test_symbols_are_exported(L):
    for name in ("aicp_hip_fov_overlap", "aicp_hip_cluster_match", "aicp_hip_alignment_features",
                 "aicp_hip_default_risk_params", "aicp_hip_last_risk_stats"):
        assert name in L.EXPORTS and hasattr(L.lib, name)
    for name in ("fov_overlap", "cluster_match", "alignment_features", "last_risk_stats"):
        assert callable(getattr(L.Context, name))


def test_default_risk_params_are_the_reference_constants(L):
    p = L.default_risk_params()
    assert p.max_angle_deg == 20.0                      # filteringUtils.cpp:258
    assert list(p.box_scale) == [1.0, 1.0, 3.0]         # :520-528
    d = L.default_prefilter()
    for k, _ in L.PrefilterParams._fields_:
        a, b = getattr(p.prefilter, k), getattr(d, k)
        assert (list(a) == list(b)) if k == "viewpoint" else (a == b), k
    assert p.prefilter.leaf_size == np.float32(0.08) and p.prefilter.normal_k == 30
    q = L.default_risk_params(angular_view=270.0, box_scale=(1, 2, 3))
    assert q.angular_view == 270.0 and list(q.box_scale) == [1.0, 2.0, 3.0]
    with pytest.raises(AttributeError):
        L.default_risk_params(nope=1)


def test_null_and_empty_arguments_are_invalid_without_a_device(L):
    P = np.zeros((4, 3), np.float32)
    cloud, keep = L.make_cloud(P)
    empty, keep2 = L.make_cloud(np.zeros((0, 3), np.float32))
    I = (C.c_double * 16)(*np.eye(4).ravel())
    ov = C.c_float()
    res = L.RiskResult()
    prm = L.default_risk_params()
    fake = C.c_void_p(1)   # never dereferenced: the argument checks come first
    lib = L.lib
    assert lib.aicp_hip_fov_overlap(None, C.byref(cloud), C.byref(cloud), I, I, 1.0, 360.0, C.byref(ov), None, None,
                                    None, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_fov_overlap(fake, C.byref(empty), C.byref(cloud), I, I, 1.0, 360.0, C.byref(ov), None, None,
                                    None, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_fov_overlap(fake, C.byref(cloud), None, I, I, 1.0, 360.0, C.byref(ov), None, None, None,
                                    None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_fov_overlap(fake, C.byref(cloud), C.byref(cloud), None, I, 1.0, 360.0, C.byref(ov), None,
                                    None, None, None) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_alignment_features(None, C.byref(prm), C.byref(cloud), C.byref(cloud), I, I, C.byref(res),
                                           None, None, None, None, 0) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_alignment_features(fake, C.byref(prm), C.byref(cloud), C.byref(empty), I, I, C.byref(res),
                                           None, None, None, None, 0) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_alignment_features(fake, None, C.byref(cloud), C.byref(cloud), I, I, C.byref(res), None, None,
                                           None, None, 0) == L.AICP_ERR_INVALID
    al = C.c_float()
    sc = (C.c_float * 3)(1, 1, 3)
    assert lib.aicp_hip_cluster_match(None, None, None, 0, None, None, 0, 20.0, sc, C.byref(al), *([None] * 11)
                                      ) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_cluster_match(fake, None, None, 5, None, None, 0, 20.0, sc, C.byref(al), *([None] * 11)
                                      ) == L.AICP_ERR_INVALID
    assert lib.aicp_hip_last_risk_stats(None, None) == L.AICP_ERR_INVALID


def _compile(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(SHIM, "stubs", "risk"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration"),
           os.path.join(SHIM, "risk_main.cpp"), "-o", out, "-L", os.path.dirname(LIB), "-laicp_hip",
           "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists(LIB), reason="needs g++ and libaicp_hip.so")
def test_shim_header_compiles_links_and_checks_arguments(tmp_path):
    """hip_alignability.hpp with -Wall -Wextra -Werror against the reference's signatures; the
    program's device-free mode sees the reference's constants and AICP_ERR_INVALID for a null
    context."""
    exe = str(tmp_path / "risk_main")
    _compile(exe)
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu ok: angle 20 scale 1 1 3" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shim_filters_run_like_the_python_wrappers(tmp_path, L):
    """App's two call sites through the header: three orthogonal planes seen from two poses give
    an FOV overlap just under 100, three matched planes and an alignability close to 100."""
    exe = str(tmp_path / "risk_main")
    _compile(exe)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split()
    vals = {out[i]: out[i + 1] for i in range(0, len(out) - 1) if out[i] in ("fov", "alignability")}
    # (the restatement on the same lattice: 10800 and 10799 accepted, one point lies at exactly
    # 180 deg; 3 clusters a side, 3 matches, alignability 98.6)
    assert 99.98 < float(vals["fov"]) < 100.0
    assert 97.0 < float(vals["alignability"]) <= 100.0
    assert "accepted 10800 10799" in r.stdout and "eig 3" in r.stdout
