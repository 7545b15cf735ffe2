"""Contrasts between two intervention levels, without a GPU: the properties of the dense restatement
(tests/contrast_restatement.py) that the GPU tests lean on, the `baseline=` parsing of the Python mirror and its refusals (all
raised before any device call), and the two symbols in the public header."""
import inspect

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import gpslc_oracle as orc

PN = orc.PREDICTION_COVARIANCE_NOISE
GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


# ---- the restatement's own properties -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
def test_restatement_is_exactly_zero_for_equal_levels(shape, bt):
    n = 24
    c = cases.make_case(n, shape, bt, S=2, seed=5)
    for a in ((0.0, 1.0) if bt else (0.6, float(np.quantile(c["T"], 0.3)))):
        exp = cr.expected_contrast(c, [a], [a])
        assert np.array_equal(exp["meanITE"], np.zeros((n, 2, 1)))
        for s in range(2):
            assert np.array_equal(exp["covITE"][s, 0], PN * np.eye(n))
        assert np.all(exp["meanSATE"] == 0.0)
        assert np.allclose(exp["varSATE"], n * PN / n ** 2, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("n", [24, 129])
def test_binary_contrast_is_the_treated_and_untreated_halves_of_the_ordinary_levels(n, shape):
    """For T in {0, 1}: f_i(1) - f_i(0) is MeanITE_i(1) where T_i == 0 (the factual term is f_i(0)) and -MeanITE_i(0) where
    T_i == 1 — against the oracle's own conditional_ite, which knows nothing of the restatement's blocks — and the SATE is
    meanSATE(1) - meanSATE(0) (each ordinary level averages an exact 0.0 over the individuals already at that level)."""
    c = cases.make_case(n, shape, True, S=2, seed=7)
    T = c["T"]
    for p in cases.samples_of(c):
        m10, C10 = cr.conditional_ite_contrast(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], T, c["Y"], 1.0, 0.0)
        m1, _ = orc.conditional_ite(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], T, c["Y"], 1.0)
        m0, _ = orc.conditional_ite(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], T, c["Y"], 0.0)
        scale = max(np.max(np.abs(m1)), np.max(np.abs(m0)))
        assert np.max(np.abs(m10[T == 0] - m1[T == 0])) <= 1e-11 * scale
        assert np.max(np.abs(m10[T == 1] + m0[T == 1])) <= 1e-11 * scale
        s10, _ = orc.conditional_sate(m10, C10)
        s1, _ = orc.conditional_sate(m1, C10)
        s0, _ = orc.conditional_sate(m0, C10)
        assert abs(s10 - (s1 - s0)) <= 1e-11 * scale
        # and the swapped pair is the negated mean with the same covariance
        m01, C01 = cr.conditional_ite_contrast(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], T, c["Y"], 0.0, 1.0)
        assert np.max(np.abs(m01 + m10)) <= 1e-13 * scale
        assert np.max(np.abs(C01 - C10)) <= 1e-12 * p.yScale


def test_contrast_covariance_is_not_what_two_ordinary_levels_give():
    """Why the feature exists: Var(SATE(a) - SATE(b)) is far from varSATE(a) + varSATE(b) (the two share the factual term
    and the whole GP)."""
    c = cases.make_case(60, "UX", False, S=1, seed=9)
    exp = cr.expected_contrast(c, [0.6], [-0.4])
    p = cases.samples_of(c)[0]
    _, va = orc.sate_distributions([p], c["X"], c["T"], c["Y"], 0.6)
    _, vb = orc.sate_distributions([p], c["X"], c["T"], c["Y"], -0.4)
    v = exp["varSATE"][0, 0]
    assert v > 0.0 and abs(v - (va[0] + vb[0])) > 0.1 * v


def test_pairs_keep_their_distance():
    for bt in (False, True):
        c = cases.make_case(200, "UX", bt, S=1, seed=3)
        for L in (1, 5, 40, 130):
            A, B = cr.pairs(c, L)
            assert A.shape == B.shape == (L,)
            assert np.all(np.abs(A - B) >= 0.25)


# ---- the Python mirror: parsing and refusals, before any device call -------------------------------------------------
def _object(gp, n=12, bt=False):
    c = cases.make_case(n, "UX", bt, S=2, seed=1)
    return cases.gpslc_object(gp, c), c


def test_baseline_is_a_keyword_of_every_estimation_entry_point():
    import causalgpslc_jl_amd as gp
    for fn in (gp.predict, gp.ITEDistributions, gp.SATEDistributions, gp.ITEsamples, gp.sampleITE, gp.sampleSATE):
        par = inspect.signature(fn).parameters
        assert "baseline" in par and par["baseline"].default is None, fn.__name__


def test_baseline_parsing():
    from causalgpslc_jl_amd import api
    assert np.array_equal(api._baseline(0.5, 3), [0.5, 0.5, 0.5])
    assert np.array_equal(api._baseline(True, 2), [1.0, 1.0])
    assert np.array_equal(api._baseline(np.float64(2.0), 1), [2.0])
    b = api._baseline([0, 1, 2], 3)
    assert b.dtype == np.float64 and b.flags.c_contiguous and np.array_equal(b, [0.0, 1.0, 2.0])
    for bad in ([0.0, 1.0], np.zeros((3, 1)), np.zeros((1, 3)), []):
        with pytest.raises(ValueError, match="L = 3"):
            api._baseline(bad, 3)


def test_baseline_refusals_come_before_any_device_call():
    import causalgpslc_jl_amd as gp
    g, c = _object(gp)
    n = c["n"]
    D = np.stack([c["T"] + 0.5, c["T"]])
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, D, baseline=0.0)                       # vector levels
    with pytest.raises(ValueError, match="scalar"):
        gp.SATEDistributions(g, c["T"] + 0.5, baseline=0.0)
    with pytest.raises(ValueError, match="scalar"):
        gp.ITEDistributions(g, c["T"] + 0.5, baseline=0.0)
    with pytest.raises(ValueError, match="scalar"):
        gp.sampleITE(g, c["T"] + 0.5, baseline=0.0)
    with pytest.raises(NotImplementedError, match="devices"):
        gp.predict(g, [0.6, 0.2], baseline=0.0, devices=[0, 0])
    with pytest.raises(ValueError, match="L = 2"):
        gp.predict(g, [0.6, 0.2], baseline=[0.0, 0.1, 0.2])
    with pytest.raises(ValueError, match="L = 1"):
        gp.ITEDistributions(g, 0.6, baseline=[0.0, 0.1])
    with pytest.raises(ValueError, match="L = 1"):
        gp.sampleSATE(g, 0.6, baseline=np.full(n, 0.1))     # a per-individual baseline is not a contrast of two levels
    assert g._ctx is None                                    # nothing above reached the device


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_header_declares_the_contrast_symbols_and_the_binding_table_has_them():
    from causalgpslc_jl_amd import _lib
    hdr = set(_lib.header_symbols())
    for name in ("gpslc_predict_contrast", "gpslc_ite_distributions_contrast"):
        assert name in hdr and name in _lib.SIGNATURES
    # one more pointer (doT_base) than gpslc_predict, one more double than gpslc_ite_distributions
    assert len(_lib.SIGNATURES["gpslc_predict_contrast"][1]) == len(_lib.SIGNATURES["gpslc_predict"][1]) + 1
    assert len(_lib.SIGNATURES["gpslc_ite_distributions_contrast"][1]) == len(_lib.SIGNATURES["gpslc_ite_distributions"][1]) + 1
    txt = open(_lib.HEADER_PATH).read()
    assert "f_i(a) - f_i(b)" in txt and "pred_noise*I" in txt and "cancel" in txt
