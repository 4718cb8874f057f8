"""CPU checks for the mapping session's built map (aicp_hip_session_keep_aligned_map, _aligned_map,
_take_aligned_map), the go-back (aicp_hip_mapsession_start_go_back) and the start on a loaded map
(aicp_hip_session_start_on_map): the entry points are declared, exported and bound, null arguments
are refused before any device work, cloud_io.load_ply_xyz reads what the node's loader reads, and
the go-back's count rule (tests/mapping_reference.py: GoBackCount) equals a brute-force App graph."""
import ctypes as C
import itertools
import os
import re
import struct

import numpy as np
import pytest

import mapping_reference as mr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"aicp_hip_session_keep_aligned_map": 3, "aicp_hip_session_aligned_map": 3,
       "aicp_hip_session_take_aligned_map": 3, "aicp_hip_mapsession_start_go_back": 4,
       "aicp_hip_session_start_on_map": 6, "aicp_hip_test_promote_map": 10}


def test_new_symbols_are_declared_exported_and_bound():
    import aicp_mapping_amd._lib as L

    header = open(os.path.join(ROOT, "include", "aicp_hip.h")).read()
    so = C.CDLL(L.LIB_PATH)
    for name, n_args in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name), name
        assert name in L.EXPORTS and name in L._NEWEST, name
        assert len(getattr(L.lib, name).argtypes) == n_args, name
    # the go-back is spelled aicp_hip_mapsession_*: the aicp_hip_map_session_* family stays at seven
    assert len(set(re.findall(r"\b(aicp_hip_map_session_\w+)\s*\(", header))) == 7
    from aicp_mapping_amd import cloud_io, prior_map
    from aicp_mapping_amd.map_session import MapSession
    from aicp_mapping_amd.session import AppSession

    assert "keep_aligned_map" in AppSession.__init__.__code__.co_varnames
    for name in ("aligned_map", "take_aligned_map", "start_on_map", "keep_aligned_map"):
        assert hasattr(AppSession, name), name
    assert hasattr(MapSession, "start_go_back")
    assert callable(cloud_io.load_ply_xyz) and callable(prior_map.load_map_from_file)


def test_null_arguments_are_refused():
    import aicp_mapping_amd._lib as L

    lib, bad = L.lib, L.AICP_ERR_INVALID
    h = C.c_void_p()
    pose = np.eye(4, dtype=F32).reshape(16)
    assert lib.aicp_hip_session_keep_aligned_map(None, None, 1) == bad
    assert lib.aicp_hip_session_aligned_map(None, None, C.byref(h)) == bad
    assert lib.aicp_hip_session_aligned_map(None, None, None) == bad
    assert lib.aicp_hip_session_take_aligned_map(None, None, C.byref(h)) == bad
    assert lib.aicp_hip_mapsession_start_go_back(None, None, None, None) == bad
    assert lib.aicp_hip_session_start_on_map(None, None, None, L._fptr(pose), -15.0, 15.0) == bad
    assert lib.aicp_hip_session_start_on_map(None, None, None, None, -15.0, 15.0) == bad
    blk = np.zeros(448, np.uint8)
    pts = np.zeros(4, F32)
    dirty = C.c_uint64()
    assert lib.aicp_hip_test_promote_map(None, 2, L._fptr(pts), 1, 0, 0, blk.ctypes.data_as(C.c_void_p), L._fptr(pts),
                                         L._fptr(pts), C.byref(dirty)) == bad


# ---- load_ply_xyz ----------------------------------------------------------------------------------
PTS = np.array([[0.5, -1.25, 3.0], [1e-3, 2.5, -7.75], [-0.0, 100.125, 1.0], [4.0, 5.0, 6.0]], np.float64)


def write_ply(path, fmt, coord="float", extra=True, face=True, face_first=False, names="xyz"):
    """Vertices of PTS with an uchar before x and a float after z (extra), and a face element."""
    n = len(PTS)
    vprops = (["property uchar tag"] if extra else []) + [f"property {coord} {a}" for a in names] + (
        ["property float intensity"] if extra else [])
    vhead = [f"element vertex {n}"] + vprops
    fhead = ["element face 2", "property list uchar int vertex_indices"] if face else []
    head = ["ply", f"format {fmt} 1.0", "comment made by the test"] + (fhead + vhead if face_first else vhead + fhead) + [
        "end_header"]
    faces = [[0, 1, 2], [1, 2, 3, 0]]
    end = ">" if fmt == "binary_big_endian" else "<"
    c = "d" if coord == "double" else "f"
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))

        def vertices():
            for i, p in enumerate(PTS):
                if fmt == "ascii":
                    row = ([str(i)] if extra else []) + [repr(float(v)) for v in p] + (["0.5"] if extra else [])
                    f.write((" ".join(row) + "\n").encode("ascii"))
                else:
                    f.write((struct.pack(end + "B", i) if extra else b"") + struct.pack(end + 3 * c, *p) +
                            (struct.pack(end + "f", 0.5) if extra else b""))

        def face_rows():
            for idx in faces if face else []:
                if fmt == "ascii":
                    f.write((" ".join(str(v) for v in [len(idx)] + idx) + "\n").encode("ascii"))
                else:
                    f.write(struct.pack(end + "B" + "i" * len(idx), len(idx), *idx))

        for part in ((face_rows, vertices) if face_first else (vertices, face_rows)):
            part()


@pytest.mark.parametrize("face_first", [False, True])
@pytest.mark.parametrize("coord", ["float", "double"])
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_load_ply_xyz_round_trips(tmp_path, fmt, coord, face_first):
    from aicp_mapping_amd.cloud_io import load_ply_xyz

    p = str(tmp_path / "map.ply")
    write_ply(p, fmt, coord=coord, face_first=face_first)
    got = load_ply_xyz(p)
    assert got.dtype == F32 and got.shape == (4, 3) and got.flags["C_CONTIGUOUS"]
    assert got.tobytes() == PTS.astype(F32).tobytes()
    write_ply(p, fmt, coord=coord, extra=False, face=False)
    assert load_ply_xyz(p).tobytes() == PTS.astype(F32).tobytes()


def test_load_ply_xyz_refuses_what_the_loader_does_not_read(tmp_path):
    from aicp_mapping_amd.cloud_io import load_ply_xyz

    p = str(tmp_path / "bad.ply")
    write_ply(p, "binary_big_endian")
    with pytest.raises(ValueError):
        load_ply_xyz(p)
    for fmt in ("ascii", "binary_little_endian"):
        write_ply(p, fmt, names="ayz")  # no x
        with pytest.raises(ValueError):
            load_ply_xyz(p)
    write_ply(p, "binary_little_endian")
    blob = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(blob[:-40])  # truncated inside the last vertex (the two faces take 30 bytes)
    with pytest.raises(ValueError):
        load_ply_xyz(p)
    with open(p, "wb") as f:
        f.write(b"# .PCD v0.7\n")
    with pytest.raises(ValueError):
        load_ply_xyz(p)
    with open(p, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError):  # no vertex element
        load_ply_xyz(p)


# ---- the go-back's count -----------------------------------------------------------------------------
@pytest.mark.parametrize("on_map", [False, True])
def test_go_back_count_equals_the_brute_force_graph(on_map):
    """Every sequence of up to 6 readings over accepted / dropped / gated, and each of them cut
    short by a reading that ends the worker (after which a go-back is refused)."""
    for n in range(7):
        for events in itertools.product("adg", repeat=n):
            c = mr.GoBackCount(on_map)
            for e in events:
                c.step(e)
            assert c.n_clouds == mr.brute_force_graph(events, on_map), events
            assert c.n_clouds == (0 if on_map else 1) + sum(e != "d" for e in events)
            c.step("e")
            assert c.ended and c.n_clouds == mr.brute_force_graph(events + ("e", "a"), on_map)
    # the phases the count decides on the prior map (rules 4, 6, 7 of tests/localization_reference.py)
    c = mr.GoBackCount(False)
    for e in "aadga":
        c.step(e)
    assert c.n_clouds == 5
    assert c.n_clouds != 0  # the drop test is live on the first localisation reading
    assert [(c.n_clouds + k) % 3 == 0 for k in range(4)] == [False, True, False, False]  # merges at frequency 3
    assert mr.GoBackCount(True).n_clouds == 0  # a start on a map with nothing accepted: App's empty graph
