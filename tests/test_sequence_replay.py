"""The paths of the two offline App-order entry points that no other test looks at:
aicp_hip_sequence_run_raw in debug mode and aicp_hip_sequence_run_risk in both modes, where a call
ends early, takes parameters the live session's constructor refuses, or shares its context.

What is pinned: the return code and *n_done on every ending; the ending reading's result,
correction and record byte for byte; that nothing past it is written (the arrays are pre-filled
with a sentinel); the wording of the context's error text; that a NaN max_correction_magnitude
accepts every reading and unknown flag bits are ignored; that a failed call leaves the context as
a fresh one; and that a caller's own AppSession on the same context is not disturbed by a whole
call in the middle of its run. Good runs are computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import risk_reference as rr
import svm_reference as sr
from aicp_mapping_amd import synthetic as sy

pytestmark = pytest.mark.gpu

RES = float(np.float32(0.2))
F32 = np.float32
SENTINEL = 0xAB
N = 4
# (entry point, debug): aicp_hip_sequence_run_raw's robot branch is the windowed stream, not this loop
VARIANTS = [("raw", True), ("risk", False), ("risk", True)]
IDS = ["raw-debug", "risk-robot", "risk-debug"]
EYE = np.eye(4, dtype=F32).tobytes()


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(L, tmp_path_factory):
    """raw = overlap - 0 >= 0, so risk <= 0.5: under threshold 1.0 the gate never closes."""
    m = L.SvmModel(sr.write_threshold_model(str(tmp_path_factory.mktemp("svm") / "thr_0.xml"), 0.0))
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def stream():
    """4 raw readings, every one accepted; at frequency 2 readings 1 and 3 become the reference."""
    return sy.make_stream(n_readings=N, n_points=20000, seed=8, half=12.0)


def scattered():
    """30 scattered points: no region of 50, the pre-filter keeps none."""
    return np.random.default_rng(4).uniform(-5, 5, size=(30, 3)).astype(F32)


def seq_params(L, debug, freq=2, max_corr=1.0, extra_flags=0):
    return L.default_sequence_params(reference_update_frequency=freq, max_correction_magnitude=max_corr,
                                     resolution=RES,
                                     flags=L.AICP_RUN_OVERLAP | (L.AICP_SEQ_DEBUG if debug else 0) | extra_flags)


def call(ctx, L, model, variant, first, first_origin, readings, origins, prm, cfg=None):
    """One call through L.lib into arrays filled with the sentinel. Returns dict(rc, done, T, res,
    rec: per reading the bytes of the correction, the result and the record, err)."""
    kind, _ = variant
    cfg = cfg or L.default_config()
    pf = L.default_prefilter()
    n = len(readings)
    fc, keep0 = L.make_cloud(first, first_origin)
    arr = (L.Cloud * n)()
    keep = [keep0]
    for i, r in enumerate(readings):
        arr[i], k = L.make_cloud(r, origins[i])
        keep.append(k)
    outT = np.zeros((n, 16), F32)
    res = (L.SequenceResult * n)()
    rec = (L.PipelineRecord * n)()
    C.memset(outT.ctypes.data, SENTINEL, outT.nbytes)
    C.memset(res, SENTINEL, C.sizeof(res))
    C.memset(rec, SENTINEL, C.sizeof(rec))
    done = C.c_size_t(77)
    if kind == "raw":
        rc = L.lib.aicp_hip_sequence_run_raw(ctx.h, C.byref(cfg), C.byref(prm), C.byref(pf), C.byref(fc), arr, n,
                                             L._fptr(outT), res, C.byref(done))
    else:
        rp = L.default_risk_params(angular_view=270.0)
        p0 = L._pose16(rr.pose(0.0, first_origin))
        pn = np.ascontiguousarray(np.concatenate([L._pose16(rr.pose(4.0 * (i + 1), origins[i])) for i in range(n)]))
        rc = L.lib.aicp_hip_sequence_run_risk(ctx.h, C.byref(cfg), C.byref(prm), C.byref(pf), C.byref(rp), model.h,
                                              1.0, C.byref(fc), L._dptr(p0), arr, L._dptr(pn), n, L._fptr(outT), res,
                                              rec, C.byref(done))
    return dict(rc=rc, done=done.value, T=[outT[i].tobytes() for i in range(n)], res=[bytes(res[i]) for i in range(n)],
                rec=[bytes(rec[i]) for i in range(n)], out=[L.SequenceResult.from_buffer_copy(res[i]) for i in range(n)],
                err=ctx.last_error())


def untouched(L, run, i, variant):
    ok = run["T"][i] == bytes([SENTINEL]) * 64 and run["res"][i] == bytes([SENTINEL]) * C.sizeof(L.SequenceResult)
    return ok and (variant[0] == "raw" or run["rec"][i] == bytes([SENTINEL]) * C.sizeof(L.PipelineRecord))


def same_call(a, b):
    return (a["rc"], a["done"], a["T"], a["res"], a["rec"]) == (b["rc"], b["done"], b["T"], b["res"], b["rec"])


_GOOD = {}


def good(L, model, variant):
    """The stream on a context of its own (computed once): the bytes every other context is held to."""
    if variant not in _GOOD:
        st = stream()
        c = L.Context(0)
        _GOOD[variant] = call(c, L, model, variant, st.first, st.first_origin, st.readings, st.origins,
                              seq_params(L, variant[1]))
        c.close()
        g = _GOOD[variant]
        assert g["rc"] == 0 and g["done"] == N
        assert [o.is_reference for o in g["out"]] == [0, 1, 0, 1] and all(o.accepted for o in g["out"])
    return _GOOD[variant]


def emptied_at_2(ctx, L, model, variant):
    st = stream()
    reads = st.readings[:2] + [scattered()] + st.readings[3:]
    return call(ctx, L, model, variant, st.first, st.first_origin, reads, st.origins, seq_params(L, variant[1]))


# ---- 1. an emptied reading at index 2 of 4 ------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_emptied_reading_mid_stream(ctx, L, model, variant):
    run = emptied_at_2(ctx, L, model, variant)
    g = good(L, model, variant)
    assert run["rc"] == L.AICP_ERR_INVALID and run["done"] == 3
    assert run["err"] == "reading 2 keeps no point after the pre-filter"
    for i in range(2):  # the readings before it are the good run's
        assert run["T"][i] == g["T"][i] and run["res"][i] == g["res"][i] and run["rec"][i] == g["rec"][i], i
    # the ending reading: a zeroed result but both statuses and the current reference (reading 1,
    # promoted at frequency 2), the identity, a zero record
    want = L.SequenceResult()
    want.status = want.icp.status = L.AICP_ERR_INVALID
    want.reference = 1
    assert run["res"][2] == bytes(want)
    assert run["T"][2] == EYE
    if variant[0] == "risk":
        assert run["rec"][2] == bytes(L.PipelineRecord())
    assert untouched(L, run, 3, variant)


# ---- 2. an emptied first cloud -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_emptied_first_cloud(ctx, L, model, variant):
    st = stream()
    run = call(ctx, L, model, variant, scattered(), st.first_origin, st.readings, st.origins,
               seq_params(L, variant[1]))
    assert run["rc"] == L.AICP_ERR_INVALID and run["done"] == 0
    assert run["err"] == "the first cloud keeps no point after the pre-filter"
    assert all(untouched(L, run, i, variant) for i in range(N))


# ---- 3. a registration status mid-stream ---------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_registration_status_mid_stream(ctx, L, model, variant):
    """tests/test_session.py::test_registration_error_ends_the_session's means: reading 2 lies 200 m
    away under a 5 m matcher radius."""
    st = stream()
    reads, origins = list(st.readings), list(st.origins)
    reads[2] = (reads[2] + F32(200.0)).astype(F32)
    origins[2] = origins[2] + 200.0
    cfg = L.default_config(nn_max_dist=5.0)
    run = call(ctx, L, model, variant, st.first, st.first_origin, reads, origins, seq_params(L, variant[1]), cfg=cfg)
    assert run["rc"] == L.AICP_ERR_CONVERGENCE and run["done"] == 3
    assert run["err"].startswith(f"reading 2: status {L.AICP_ERR_CONVERGENCE}: ")
    assert [o.status for o in run["out"][:2]] == [0, 0]
    o = run["out"][2]
    assert o.status == o.icp.status == L.AICP_ERR_CONVERGENCE and not o.accepted and not o.is_reference
    assert o.reference == 1
    if variant[0] == "risk":
        rec = L.PipelineRecord.from_buffer_copy(run["rec"][2])
        assert rec.registered == 1 and rec.n_read > 0 and o.icp.overlap_percent == rec.octree_overlap
    assert untouched(L, run, 3, variant)


# ---- 4. parameters the live session's constructor refuses ------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_nan_bound_and_unknown_flag_bits(ctx, L, model, variant):
    """tests/test_session.py's raw fixture cut to 4 readings: reading 3 carries a 0.8 m jump, which a
    0.4 m bound drops."""
    st = sy.make_stream(n_readings=N, n_points=20000, seed=8, half=12.0, jumps={3: (0, -0.8, 0)})

    def run(**kw):
        return call(ctx, L, model, variant, st.first, st.first_origin, st.readings, st.origins,
                    seq_params(L, variant[1], freq=5, **kw))

    odd, clean, tight = run(max_corr=float("nan"), extra_flags=1 << 20), run(max_corr=1e30), run(max_corr=0.4)
    assert odd["rc"] == clean["rc"] == tight["rc"] == 0 and odd["done"] == clean["done"] == tight["done"] == N
    assert [o.accepted for o in tight["out"]] == [1, 1, 1, 0]
    assert all(o.accepted for o in odd["out"])
    assert same_call(odd, clean)


# ---- 5. a failed call, then a good one --------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_good_call_after_a_failed_one(L, model, variant):
    st = stream()
    c = L.Context(0)
    failed = emptied_at_2(c, L, model, variant)
    assert failed["rc"] == L.AICP_ERR_INVALID and failed["done"] == 3
    again = call(c, L, model, variant, st.first, st.first_origin, st.readings, st.origins, seq_params(L, variant[1]))
    c.close()
    assert same_call(again, good(L, model, variant))


# ---- 6. a caller's session around a whole call ------------------------------------------------------------
def test_callers_session_is_not_disturbed(ctx, L, model):
    from aicp_mapping_amd.session import AppSession

    st = stream()
    variant = ("raw", True)

    def feed(between):
        s = AppSession(ctx, params=seq_params(L, True), prefilter=True)
        s.start(st.first, st.first_origin)
        got = []
        for i in range(N):
            if i == 2:
                between()
            T, res, kept = s.process(st.readings[i], st.origins[i])
            got.append((T.tobytes(), res, kept, s.state()["initial_T"].tobytes(), s.reference()[0].tobytes()))
        s.close()
        return got

    def whole_call():
        run = call(ctx, L, model, variant, st.first, st.first_origin, st.readings, st.origins, seq_params(L, True))
        assert same_call(run, good(L, model, variant))

    assert feed(whole_call) == feed(lambda: None)
