"""The registration quality monitor's entry points without a device: exports, defaults, struct
layouts against the header, and the argument checks that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aicp_hip.h")


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


def test_symbols_are_exported(L):
    for name in ("aicp_hip_default_monitor_params", "aicp_hip_monitor", "aicp_hip_monitor_batch",
                 "aicp_hip_last_monitor_stats"):
        assert name in L.EXPORTS and hasattr(L.lib, name)
    for name in ("monitor", "monitor_batch", "last_monitor_stats"):
        assert callable(getattr(L.Context, name))


def test_defaults_are_the_reference_constants(L):
    p = L.default_monitor_params()
    assert p.quantile == np.float32(0.60)        # icpMonitor.cpp:31
    assert p.max_accepted_dist == 0.20           # :128
    assert p.flags == 0
    q = L.default_monitor_params(quantile=0.5, flags=L.AICP_MON_PAIRED)
    assert q.quantile == 0.5 and q.flags == 1
    with pytest.raises(AttributeError):
        L.default_monitor_params(nope=1)


def header_struct(name):
    """Field (type, name, count) triples of `typedef struct { ... } name;` in the header."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for item in rest.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            out.append((ctype, m.group(1), int(m.group(2) or 1)))
    return out


CTYPES = {"float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "uint64_t": C.c_uint64}


@pytest.mark.parametrize("cname,pyname,size", [("aicp_monitor_params", "MonitorParams", 24),
                                               ("aicp_monitor_result", "MonitorResult", 56),
                                               ("aicp_monitor_stats", "MonitorStats", 40)])
def test_ctypes_structs_have_the_headers_layout(L, cname, pyname, size):
    """The same fields in the same order with the same types; natural alignment then gives both
    sides the same offsets, and the size is the header's."""
    fields = header_struct(cname)
    cls = getattr(L, pyname)
    assert [(n, CTYPES[t] if k == 1 else CTYPES[t] * k) for t, n, k in fields] == [(n, t) for n, t in cls._fields_]
    assert C.sizeof(cls) == size
    if cname == "aicp_monitor_result":   # no implicit padding: the fields fill the struct
        assert sum(C.sizeof(t) for _, t in cls._fields_) == size


def test_null_arguments_are_invalid_without_a_device(L):
    P = np.zeros((4, 3), np.float32)
    cloud, keep = L.make_cloud(P)
    prm = L.default_monitor_params()
    res = L.MonitorResult()
    st = L.MonitorStats()
    pair, keep2 = L.make_pair(P, P)
    fake = C.c_void_p(1)   # never dereferenced: the null checks come first
    lib = L.lib
    inv = L.AICP_ERR_INVALID
    assert lib.aicp_hip_monitor(None, C.byref(prm), None, C.byref(cloud), C.byref(cloud), None, C.byref(res), None,
                                None) == inv
    assert lib.aicp_hip_monitor(fake, None, None, C.byref(cloud), C.byref(cloud), None, C.byref(res), None, None) == inv
    assert lib.aicp_hip_monitor(fake, C.byref(prm), None, None, C.byref(cloud), None, C.byref(res), None, None) == inv
    assert lib.aicp_hip_monitor(fake, C.byref(prm), None, C.byref(cloud), None, None, C.byref(res), None, None) == inv
    assert lib.aicp_hip_monitor(fake, C.byref(prm), None, C.byref(cloud), C.byref(cloud), None, None, None, None) == inv
    assert lib.aicp_hip_monitor_batch(None, C.byref(prm), None, C.byref(pair), 1, None, C.byref(res)) == inv
    assert lib.aicp_hip_monitor_batch(fake, C.byref(prm), None, None, 1, None, C.byref(res)) == inv
    assert lib.aicp_hip_monitor_batch(fake, C.byref(prm), None, C.byref(pair), 1, None, None) == inv
    assert lib.aicp_hip_last_monitor_stats(None, C.byref(st)) == inv
    lib.aicp_hip_default_monitor_params(None)   # a null pointer is ignored


def test_source_hash_covers_the_monitor_sources(L):
    """The provenance hash reads its file list from the Makefile: the new sources are in it."""
    mk = open(os.path.join(ROOT, "aicp_mapping_amd", "csrc", "Makefile")).read()
    assert "kernels_monitor.hip" in mk and "monitor.cpp" in mk
    assert L.provenance()["built_from_tree"] or os.environ.get("AICP_HIP_LIB")
