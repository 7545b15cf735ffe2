"""Marginal effects (the slope d f_i(t) / dt at a scalar level), without a GPU: the dense restatement
(tests/slope_restatement.py) against the finite difference of contrasts it is the limit of, the structured forms the library
uses against the dense blocks, the `slope=` keyword of the Python mirror with its refusals (all raised before any device call),
and the two symbols in the public header."""
import inspect

import numpy as np
import pytest

import cases
import gpslc_oracle as orc
import slope_restatement as sr

PN = orc.PREDICTION_COVARIANCE_NOISE


# ---- the restatement is the derivative ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,seed,a", sr.FD_CASES)
def test_central_difference_of_contrasts_converges_at_second_order(n, shape, seed, a):
    """contrast(a + h, a - h) / (2h), covariance / (4h^2), against the restatement's slope: the error at h = 1e-2 is 100 times
    the error at h = 1e-3 (within 80 ... 120) for MeanITE, CovITE, the average and its variance — a restatement with a wrong
    cross or prior block converges to something else and the ratio is 1.  The errors at h = 1e-3 are the record the GPU
    finite-difference test takes its bound from."""
    c = cases.make_case(n, shape, False, S=2, seed=seed)
    e2, e3 = sr.fd_errors(c, a, 1e-2), sr.fd_errors(c, a, sr.FD_H)
    print(f"n={n} {shape}: errors at h=1e-3 {e3.tolist()}  ratios {(e2 / e3).tolist()}")
    assert np.all(e2 / e3 >= 80.0) and np.all(e2 / e3 <= 120.0)
    rec = np.array(sr.FD_MEASURED[(n, shape)])
    worst = e3.max(axis=0)
    assert np.all(worst <= rec * 1.001) and np.all(worst >= rec * 0.999), (worst, rec)


# ---- the structured forms against the dense blocks ------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("n", [24, 129])
def test_structured_curve_covariance_equals_the_dense_sum(n, shape):
    """P_ll' - v_l . v_l' with P_ll' = (2 w - 4 (a_l - a_l')^2 w^2) rho(a_l, a_l') beta against w' Cov(g(a_l), g(a_l') | Y) w summed
    over dense n x n blocks; the diagonal against the per-level variance w' (CovITE + pred_noise I) w of expected_slope; the
    plain form's mean and variance against conditional_sate of the dense blocks.  Bounds: 1e-11 of the variance scale — the
    two sides differ by rounding only (measured 2.3e-15 here, 2.3e-13 at n = 400)."""
    c = cases.make_case(n, shape, False, S=2, seed=3)
    A = sr.levels(c, 5)
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n) / n
    exp = sr.expected_slope(c, A)
    for s in range(c["S"]):
        m, cv = sr.literal_slope_curve(c, s, A, w)
        ms, cs = sr.structured_slope_curve(c, s, A, w)
        scale = np.max(np.abs(np.diag(cs)))
        assert np.max(np.abs(m[:, 0] - ms)) <= 1e-11 * np.max(np.abs(ms))
        assert np.max(np.abs(cv[:, :, 0] - cs)) <= 1e-11 * scale
        assert np.array_equal(cs, cs.T)
        for l, a in enumerate(A):
            var_l = float(w @ exp["covITE"][s, l] @ w)
            assert abs(cs[l, l] - var_l) <= 1e-11 * scale
            assert abs(ms[l] - float(w @ exp["meanITE"][:, s, l])) <= 1e-11 * np.max(np.abs(ms))
            pm, pv = sr.structured_slope_average(c, s, a)
            assert abs(pm - exp["meanSATE"][s, l]) <= 1e-11 * abs(exp["meanSATE"][s, l])
            assert abs(pv - exp["varSATE"][s, l]) <= 1e-11 * exp["varSATE"][s, l]


def test_slope_covariance_without_features_is_semi_definite_to_rounding():
    """Shape "T": B is constant, so CovITE has rank one up to rounding and its smallest eigenvalue is a rounding-level
    negative number — the draws need the robust factorisation (and get the pred_noise jitter first, as every CovITE)."""
    c = cases.make_case(129, "T", False, S=2, seed=3)
    exp = sr.expected_slope(c, [0.4])
    for s in range(2):
        ev = np.linalg.eigvalsh(exp["covITE"][s, 0] - PN * np.eye(129))
        assert abs(ev[0]) <= 1e-11 * ev[-1]


def test_levels_helper():
    for bt in (False, True):
        c = cases.make_case(50, "UX", bt, S=1, seed=3)
        for L in (1, 5, 40, 130):
            A = sr.levels(c, L)
            assert A.shape == (L,) and np.all(np.isfinite(A))


# ---- the Python mirror: the keyword and its refusals, before any device call ----------------------------------------
def test_slope_is_a_keyword_of_every_estimation_entry_point():
    import causalgpslc_jl_amd as gp
    for fn in (gp.predict, gp.ITEDistributions, gp.SATEDistributions, gp.ITEsamples, gp.sampleITE, gp.sampleSATE,
               gp.effectCurve, gp.sampleEffectCurve):
        par = inspect.signature(fn).parameters
        assert "slope" in par and par["slope"].default is False, fn.__name__


def test_slope_refusals_come_before_any_device_call():
    import causalgpslc_jl_amd as gp
    c = cases.make_case(12, "UX", False, S=2, seed=1)
    g = cases.gpslc_object(gp, c)
    D = np.stack([c["T"] + 0.5, c["T"]])
    w = np.full(12, 1.0 / 12)
    for fn, args in ((gp.predict, ([0.6, 0.2],)), (gp.SATEDistributions, (0.6,)), (gp.ITEDistributions, (0.6,)),
                     (gp.ITEsamples, (0.6, 2)), (gp.sampleITE, (0.6,)), (gp.sampleSATE, (0.6,)), (gp.effectCurve, ([0.6, 0.2],)),
                     (gp.sampleEffectCurve, ([0.6, 0.2],))):
        with pytest.raises(ValueError, match="baseline"):
            fn(g, *args, slope=True, baseline=0.0)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, D, slope=True)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, D, slope=True, weights=w)
    for fn in (gp.SATEDistributions, gp.ITEDistributions, gp.sampleITE, gp.sampleSATE):
        with pytest.raises(ValueError, match="scalar levels"):
            fn(g, c["T"] + 0.5, slope=True)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.effectCurve(g, D, slope=True)
    with pytest.raises(ValueError, match="devices"):
        gp.predict(g, [0.6, 0.2], slope=True, devices=[0, 0])
    with pytest.raises(ValueError, match="devices"):
        gp.effectCurve(g, [0.6, 0.2], slope=True, devices=[0])
    with pytest.raises(ValueError, match="devices"):
        gp.sampleEffectCurve(g, [0.6, 0.2], slope=True, devices=[0])
    assert g._ctx is None                                    # nothing above reached the device


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_header_declares_the_slope_symbols_and_the_binding_table_has_them():
    from causalgpslc_jl_amd import _lib
    hdr = set(_lib.header_symbols())
    for name in ("gpslc_predict_slope", "gpslc_ite_distributions_slope"):
        assert name in hdr and name in _lib.SIGNATURES
    # gpslc_predict_curve without the baseline pointer; gpslc_ite_distributions' own signature
    assert len(_lib.SIGNATURES["gpslc_predict_slope"][1]) == len(_lib.SIGNATURES["gpslc_predict_curve"][1]) - 1
    assert _lib.SIGNATURES["gpslc_ite_distributions_slope"] == _lib.SIGNATURES["gpslc_ite_distributions"]
    txt = open(_lib.HEADER_PATH).read()
    assert "d f_i(t) / dt" in txt and "2 (T_j - a) wt r^a_j" in txt
