"""The classifier's kernel (aicp_hip_svm_predict, kernels_svm.hip) against the restatement
tests/svm_reference.py and against the reference's own recordings (tests/golden/svm).

Bars, all computed from the restatement's alpha and K, never from the device's output:
  raw against the restatement: ulp32(raw_ref) + 2^-23 max_k |alpha_k| K_k (the one float rounding of
    the sum; one K landing on the neighbouring float; the double sum's reordering, about 2^-45
    relative, disappears in either);
  risk against the recording: half a unit of the recorded value's sixth significant digit + 1/4
    (ulp32(raw) + 2^-23 sum_k |alpha_k| K_k) (the print rounding; the float roundings of raw and of
    every K through the logistic, whose slope is at most 1/4);
  risk against the restatement (the shape cases): 1/4 of the raw bar + 1e-15 (exp and the division
    in double on both sides).
tests/test_svm_cpu.py holds what needs no device."""
import numpy as np
import pytest

import svm_reference as sr

pytestmark = pytest.mark.gpu


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
def golden(L):
    """name -> model (library), restatement on the 269 recorded inputs, recording; read only."""
    X = sr.read_inputs()
    out = {}
    for name, (model_file, probs_file, n_above) in sr.MODELS.items():
        ref = sr.read_model(sr.golden(model_file))
        raw, risk, terms = sr.predict(ref, X)
        rec, texts = sr.read_probs(sr.golden(probs_file))
        out[name] = dict(model=L.SvmModel(sr.golden(model_file)), X=X, raw=raw, risk=risk, terms=terms, rec=rec,
                         texts=texts, n_above=n_above)
    yield out
    for g in out.values():
        g["model"].close()


@pytest.mark.parametrize("name", sorted(sr.MODELS))
def test_golden_models_against_restatement_and_recording(ctx, golden, name):
    g = golden[name]
    raw, risk = ctx.svm_predict(g["model"], g["X"])
    bar_raw = sr.raw_bar(g["raw"], g["terms"])
    bar_rec = sr.recorded_bar(g["raw"], g["terms"], g["texts"])
    e_raw = np.abs(raw.astype(np.float64) - g["raw"].astype(np.float64))
    e_rec = np.abs(risk - g["rec"])
    print(f"{name}: |raw_dev - raw_ref| max {e_raw.max():.3g} (bar at it {bar_raw[np.argmax(e_raw)]:.3g}), "
          f"|risk_dev - recorded| max {e_rec.max():.3g} (bar max {bar_rec.max():.3g}), "
          f"restatement vs recorded max {np.abs(g['risk'] - g['rec']).max():.3g}")
    assert (e_raw <= bar_raw).all()
    assert (e_rec <= bar_rec).all()
    gated = sr.gate(risk, 0.5)
    assert np.array_equal(gated, g["rec"] > 0.5)
    assert int(gated.sum()) == g["n_above"]


def shape_model(tmp_path, count, index_kind, seed):
    rng = np.random.default_rng(seed)
    total = count if index_kind == "absent" else count + 3
    sv = rng.uniform(0.0, 100.0, size=(total, 2)).astype(np.float32)
    alpha = rng.uniform(0.02, 0.1, size=count) * rng.choice([-1.0, 1.0], size=count)
    index = None if index_kind == "absent" else rng.permutation(total)[:count]
    path = sr.write_model(str(tmp_path / f"m_{count}_{index_kind}.xml"), sv, alpha, 0.0123, 3.43, 1.5e-4, 0.1,
                          index=index, sv_total=total, fmt=3 if count % 2 else 0)
    return path


@pytest.mark.parametrize("index_kind", ["permutation", "absent"])
@pytest.mark.parametrize("count", [1, 13, 63, 64, 65, 200])
def test_shapes(ctx, L, tmp_path, count, index_kind):
    """Decision functions of one entry, less than a wave, a wave and its neighbours, several strides;
    1 sample, a workgroup's four and its neighbours' counts, and 4097 in one call (1025 workgroups).
    A sample's result does not depend on the batch it is in."""
    path = shape_model(tmp_path, count, index_kind, seed=100 + count)
    ref = sr.read_model(path)
    assert ref["sv_count"] == count and ref["has_index"] == (index_kind != "absent")
    model = L.SvmModel(path)
    rng = np.random.default_rng(count)
    X = np.stack([rng.uniform(0, 100, 4097), rng.uniform(0, 90, 4097)], 1).astype(np.float32)
    raw_ref, risk_ref, terms = sr.predict(ref, X)
    bar = sr.raw_bar(raw_ref, terms)
    whole = None
    for n in (4097, 1, 63, 64, 65):
        raw, risk = ctx.svm_predict(model, X[:n])
        assert raw.shape == (n,) and risk.shape == (n,)
        assert (np.abs(raw.astype(np.float64) - raw_ref[:n].astype(np.float64)) <= bar[:n]).all(), n
        assert (np.abs(risk - risk_ref[:n]) <= 0.25 * bar[:n] + 1e-15).all(), n
        if whole is None:
            whole = (raw.copy(), risk.copy())
        assert raw.tobytes() == whole[0][:n].tobytes() and risk.tobytes() == whole[1][:n].tobytes(), n
    model.close()


def test_repeat_and_second_context_give_identical_bytes(ctx, L, golden):
    g = golden["opencv3"]
    raw0, risk0 = ctx.svm_predict(g["model"], g["X"])
    raw1, risk1 = ctx.svm_predict(g["model"], g["X"])        # the model's device copy is reused
    assert raw0.tobytes() == raw1.tobytes() and risk0.tobytes() == risk1.tobytes()
    other = L.Context(0)
    try:
        raw2, risk2 = other.svm_predict(g["model"], g["X"])
        assert raw0.tobytes() == raw2.tobytes() and risk0.tobytes() == risk2.tobytes()
        # two models alternating on one context: each keeps its own device copy
        h = golden["thresh60"]
        a = other.svm_predict(h["model"], h["X"])
        b = other.svm_predict(g["model"], g["X"])
        c = other.svm_predict(h["model"], h["X"])
        assert b[0].tobytes() == raw0.tobytes() and a[1].tobytes() == c[1].tobytes()
    finally:
        other.close()


def test_nan_and_empty(ctx, L, golden):
    """A negative base under a fractional degree is NaN in pow: raw and risk are NaN and the gate
    fires; no sample is no work."""
    g = golden["opencv3"]
    raw, risk = ctx.svm_predict(g["model"], np.array([[-1.0e6, 0.0], [50.0, 10.0]], np.float32))
    assert np.isnan(raw[0]) and np.isnan(risk[0]) and sr.gate(risk, 0.5)[0]
    assert np.isfinite(risk[1])
    raw, risk = ctx.svm_predict(g["model"], np.zeros((0, 2), np.float32))
    assert raw.shape == (0,) and risk.shape == (0,)
