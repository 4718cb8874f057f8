"""k_session_promote_map and k_session_gate_promote_map alone (aicp_hip_test_promote_map), on made-up
records: the reference buffer and the map's tail hold the same bytes, numpy's restatement of apply4
(moved) or the input's bytes (gated); the header, the record and the count are what
k_session_promote / k_session_gate_promote write on the same block; with append / gate 0 not a byte
of the reference buffer, the map or the guard words is written.

Sizes: one point, one short of a block, a block, one past it, and two blocks and one point; tails 0,
1 and 255 points (the map's tail 16-byte aligned only, and at an odd point of a block)."""
import ctypes as C

import numpy as np
import pytest

from session_risk_reference import apply4

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [1, 255, 256, 257, 513]
TAILS = [0, 1, 255]
FILL = 0xA5
O_COUNT, O_REC, O_HDR, O_GATE, O_T, O_ORG = 64, 128, 192, 280, 320, 384


@pytest.fixture(scope="module")
def L():
    import aicp_mapping_amd._lib as L

    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def correction():
    """A rotation about a skew axis and a translation, float32, row-major."""
    a = np.array([0.3, -0.5, 0.81], np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = 0.37
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = [0.25, -1.5, 0.125]
    return T.astype(F32)


def reading(n):
    rng = np.random.default_rng(1000 + n)
    p = np.ones((n, 4), F32)
    p[:, :3] = rng.uniform(-20, 20, (n, 3)).astype(F32)
    p[0, 0] = F32(-0.0)
    p[n // 2, 1] = F32(-0.0)
    p[n - 1, 2] = np.array([1], np.uint32).view(F32)[0]  # the smallest denormal
    p[n // 3, 0] = np.array([0x00400000], np.uint32).view(F32)[0]  # a larger one
    return p


def block(flag, gated, T):
    """The session's block before the launch: a record the commit would have left (moved) or stale
    words (gated), a stale header, count 3, the correction (moved) or stale words (gated)."""
    b = np.zeros(448, np.uint8)
    b[0:64] = np.frombuffer((np.eye(4, dtype=F32) * F32(2)).tobytes(), np.uint8)  # initialT_: never written
    b[O_COUNT:O_COUNT + 4] = np.frombuffer(np.int32(3).tobytes(), np.uint8)
    rec = np.array([0, 1, 0 if gated else flag, 0], np.int32) if not gated else np.array([7, 7, 7, 7], np.int32)
    b[O_REC:O_REC + 16] = np.frombuffer(rec.tobytes(), np.uint8)
    b[O_REC + 16:O_REC + 40] = np.frombuffer(np.array([1.5, -2.25, 0.75]).tobytes(), np.uint8)
    b[O_HDR:O_HDR + 8] = np.frombuffer(np.array([99, 42], np.int32).tobytes(), np.uint8)
    b[O_HDR + 16:O_HDR + 40] = np.frombuffer(np.array([9.0, 9.0, 9.0]).tobytes(), np.uint8)
    b[O_GATE:O_GATE + 4] = np.frombuffer(np.int32(flag if gated else 0).tobytes(), np.uint8)
    Tcol = np.ascontiguousarray(T.T) if not gated else np.full((4, 4), 5, F32)
    b[O_T:O_T + 64] = np.frombuffer(Tcol.tobytes(), np.uint8)
    b[O_ORG:O_ORG + 24] = np.frombuffer(np.array([-3.5, 4.25, 0.7]).tobytes(), np.uint8)
    return b


def launch(ctx, L, kernel, read, tail, blk, ident=17):
    n = len(read)
    b = blk.copy()
    ref = np.zeros((n, 4), F32)
    mp = np.zeros((tail + n, 4), F32)
    dirty = C.c_uint64(123)
    ctx.check(L.lib.aicp_hip_test_promote_map(ctx.h, kernel, L._fptr(read), n, tail, ident, b.ctypes.data_as(C.c_void_p),
                                              L._fptr(ref), L._fptr(mp), C.byref(dirty)))
    return ref, mp, b, dirty.value


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("gated", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_promote_map_kernels(ctx, L, n, gated, flag):
    T = correction()
    read = reading(n)
    blk = block(flag, gated, T)
    want = read if gated else np.concatenate([apply4(T, read[:, :3]), np.ones((n, 1), F32)], 1)
    # the parent's kernel on the same block: the block it leaves and its reference buffer
    ref0, map0, blk0, dirty0 = launch(ctx, L, 1 if gated else 0, read, 0, blk)
    assert dirty0 == 0 and untouched(map0)
    for tail in TAILS:
        ref, mp, b, dirty = launch(ctx, L, 3 if gated else 2, read, tail, blk)
        assert dirty == 0, (tail, dirty)  # the guard words on both sides, and the reading's bytes
        assert b.tobytes() == blk0.tobytes(), tail  # header, record, count, T: the parent's
        assert untouched(mp[:tail]), tail  # the map before its tail
        if not flag:
            assert untouched(ref) and untouched(mp), tail
            continue
        assert ref.tobytes() == mp[tail:].tobytes(), tail
        assert ref.tobytes() == ref0.tobytes() == want.tobytes(), tail
    # what the parent's kernel left on the block, in the header's terms
    i32, f64 = blk0.view(np.int32), blk0.view(np.float64)
    assert blk0[0:64].tobytes() == blk[0:64].tobytes()  # initialT_ is never written
    if not flag:
        assert i32[O_REC // 4 + 2] == 0  # append
        changed = np.flatnonzero(blk0 != blk)
        assert set(changed) <= set(range(O_REC + 8, O_REC + 12)), changed
        return
    assert list(i32[O_HDR // 4:O_HDR // 4 + 2]) == [n, 17]
    if gated:
        assert list(i32[O_REC // 4:O_REC // 4 + 4]) == [0, 1, 1, 0] and i32[O_COUNT // 4] == 0
        assert list(f64[O_REC // 8 + 2:O_REC // 8 + 5]) == [-3.5, 4.25, 0.7] == list(f64[O_HDR // 8 + 2:O_HDR // 8 + 5])
        assert blk0[O_T:O_T + 64].tobytes() == np.eye(4, dtype=F32).tobytes()
    else:
        assert list(f64[O_HDR // 8 + 2:O_HDR // 8 + 5]) == [1.5, -2.25, 0.75] and i32[O_COUNT // 4] == 3
        assert blk0[O_REC:O_REC + 40].tobytes() == blk[O_REC:O_REC + 40].tobytes()


def test_invalid_arguments(ctx, L):
    read = reading(4)
    blk = block(1, 0, correction())
    out = np.zeros((8, 4), F32)
    dirty = C.c_uint64()
    args = (L._fptr(read), 4, 0, 0, blk.ctypes.data_as(C.c_void_p), L._fptr(out), L._fptr(out), C.byref(dirty))
    assert L.lib.aicp_hip_test_promote_map(ctx.h, 4, *args) == L.AICP_ERR_INVALID
    assert L.lib.aicp_hip_test_promote_map(ctx.h, -1, *args) == L.AICP_ERR_INVALID
    assert L.lib.aicp_hip_test_promote_map(ctx.h, 2, L._fptr(read), 0, 0, 0, *args[4:]) == L.AICP_ERR_INVALID
