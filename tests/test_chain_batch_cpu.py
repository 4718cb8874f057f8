"""The batch form of the sampled chains without a GPU: the restatement of the device's
segment rule equals the cloud-by-cloud reference on every case the GPU tests run, every way the
batch form can go wrong is caught by one of those cases, and the new calls refuse a null context
before any device work."""
import ctypes as C

import numpy as np
import pytest

import chain_batch_reference as cb
import chain_reference as cr


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


def test_the_cases_hold_what_the_batch_form_needs():
    cases = cb.cases()
    sizes = [len(c) for c in cases["ragged_random"]["clouds"]]
    assert sorted(sizes) == [1, 63, 65, 1023, 1025, 4097]
    ends = np.cumsum(sizes)[:-1]
    assert any(e % 64 for e in ends) and any(e % 1024 and e > 1024 for e in ends)   # inside a wave, inside a tile
    # points exactly on the radius
    on = [np.sqrt((c.astype(np.float64) ** 2).sum(1)) == cr.RADIUS for c in cases["ragged_radius"]["clouds"]]
    assert sum(int(o.sum()) for o in on) > 1000
    for name in cases:
        assert all(len(c) <= 4097 for c in cases[name]["clouds"]) and len(cases[name]["clouds"]) <= 8, name


@pytest.mark.parametrize("name", sorted(cb.cases()))
def test_unmutated_simulate_equals_the_reference_cloud_by_cloud(oracle, name):
    case = cb.cases()[name]
    got = cb.simulate(case)
    assert cb.mismatches(case, got) == []
    want = cb.expected(case)
    if name == "emptied_middle":
        assert [w["n"] for w in want][2] == 0 and [w["n"] for w in want][4] == 0 and want[3]["n"] > 100
    if name == "mindist_density":
        assert want[1]["counts"][0] == 0 and want[0]["n"] > 100 and want[2]["n"] > 50
    if name == "density_maxima":
        dens = cb.oracle_densities(case)
        tops = [float(d.max()) for d in dens]
        assert len(set(tops)) == len(tops), tops                      # different maxima
        assert np.all(dens[1] == dens[1][0]) and want[1]["n"] == 0    # the cube: every point saturated, all dropped
        assert all(w["n"] > 0 for k, w in enumerate(want) if k != 1)


@pytest.mark.parametrize("mut", cb.MUTATIONS)
def test_every_mutation_is_caught_by_a_gpu_case(oracle, mut):
    caught = [name for name, case in sorted(cb.cases().items()) if cb.mismatches(case, cb.simulate(case, mut))]
    print(mut, "caught by", caught)
    assert caught, mut


def test_new_calls_refuse_a_null_context(L):
    ch, cfg = L.Chain(), L.default_config()
    pts = np.ones((4, 3), np.float32)
    p, keep = L.make_pair(pts, pts)
    T = np.zeros(16, np.float32)
    assert L.lib.aicp_hip_align_chain_batch(None, C.byref(cfg), C.byref(ch), C.byref(p), 1, 0.2, L.AICP_RUN_ICP,
                                            L._fptr(T), None, None) == L.AICP_ERR_INVALID
    counts = np.array([4], np.uint32)
    oc, on, idx = np.zeros(4, np.uint64), np.zeros(1, np.uint64), np.zeros(4, np.int32)
    u64 = C.POINTER(C.c_uint64)
    assert L.lib.aicp_hip_test_chain_batch(None, C.byref(ch), 0, 1, counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           L._fptr(pts), oc.ctypes.data_as(u64), on.ctypes.data_as(u64),
                                           idx.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == L.AICP_ERR_INVALID
