"""Potential outcomes (the response surface f_i(a) itself, at a scalar or a per-individual level), without a GPU: the dense
restatement (tests/outcome_restatement.py) against the identities that tie it to the estimands the library already has, the
structured forms the library uses against the dense blocks, the `outcome=` keyword of the Python mirror with its refusals (all
raised before any device call), and the four symbols in the public header and both binding tables."""
import inspect
import os
import re

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import gpslc_oracle as orc
import outcome_restatement as ot
import vector_restatement as vr

PN = orc.PREDICTION_COVARIANCE_NOISE
SYMBOLS = ("gpslc_predict_outcome", "gpslc_predict_outcome_vec", "gpslc_ite_distributions_outcome",
           "gpslc_ite_distributions_outcome_vec")


def _args(p, c):
    return (p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"])


# ---- the restatement against the estimands that exist ---------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("bt", [False, True])
def test_ordinary_mean_ite_is_the_outcome_minus_the_fitted_surface(shape, bt):
    """MeanITE = (CovWWs' - CovWW) alpha = outcome - K alpha, and K alpha = Y - yNoise alpha: to rounding of the two dense
    products (1e-12 of the larger side)."""
    c = cases.make_case(129, shape, bt, S=2, seed=5)
    for p in cases.samples_of(c):
        for a in ot.levels(c, 3):
            m_ord, _ = orc.conditional_ite(*_args(p, c), a)
            m_out, _ = ot.conditional_outcome(*_args(p, c), a)
            CovWWp = orc.likelihood_distribution(*_args(p, c), a)[3]
            alpha = orc._sym_solve(CovWWp, c["Y"])
            fitted = c["Y"] - p.yNoise * alpha
            assert np.max(np.abs(m_ord - (m_out - fitted))) <= 1e-12 * max(np.max(np.abs(m_out)), np.max(np.abs(fitted)))


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_difference_of_two_outcomes_is_the_contrast(shape):
    c = cases.make_case(129, shape, False, S=2, seed=6)
    a, b = 0.6, -0.4
    for p in cases.samples_of(c):
        ma, _ = ot.conditional_outcome(*_args(p, c), a)
        mb, _ = ot.conditional_outcome(*_args(p, c), b)
        mc, _ = cr.conditional_ite_contrast(*_args(p, c), a, b)
        assert np.max(np.abs((ma - mb) - mc)) <= 1e-12 * max(np.max(np.abs(ma)), np.max(np.abs(mb)))


@pytest.mark.parametrize("n,shape", [(24, "UX"), (129, "T"), (129, "X")])
def test_outcome_curve_covariance_gives_the_contrast_variance(n, shape):
    """Var(w' (f(a_l) - f(a_l'))) = cov[l, l] + cov[l', l'] - 2 cov[l, l'] of the weighted outcome curve, against the contrast
    restatement's w' CovITE w.  The outcome curve carries pred_noise w.w once per level (two in the sum), the contrast once.
    Bound: 1e-11 of the larger of the curve's variances (the sum cancels against it)."""
    c = cases.make_case(n, shape, False, S=2, seed=7)
    A = ot.levels(c, 3)
    w = np.random.default_rng(n).standard_normal(n) / n
    ww = float(w @ w)
    for s, p in enumerate(cases.samples_of(c)):
        _, cov = ot.literal_outcome_curve(c, s, A, w)
        cov = cov[:, :, 0]
        scale = np.max(np.abs(np.diag(cov)))
        for l in range(3):
            for lp in range(l):
                _, Cc = cr.conditional_ite_contrast(*_args(p, c), A[l], A[lp])
                ref = float(w @ orc._symmetric_upper(Cc) @ w) + PN * ww
                got = (cov[l, l] + cov[lp, lp] - 2.0 * cov[l, lp]) - PN * ww
                assert abs(got - ref) <= 1e-11 * scale, (s, l, lp, got, ref)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("bt", [False, True])
def test_vector_level_at_the_observed_treatment_is_the_fitted_surface(shape, bt):
    """d = T: CovWWs == CovWW and CovWsWs == CovWW bit for bit, so the mean is K alpha and the covariance CovC11."""
    c = cases.make_case(50, shape, bt, S=2, seed=8)
    for p in cases.samples_of(c):
        m, C = ot.conditional_outcome_vec(*_args(p, c), c["T"].copy())
        Y, CovWW, _, CovWWp, C11, _, _, _ = orc.likelihood_distribution(*_args(p, c), 0.3)
        assert np.array_equal(m, CovWW.T @ orc._sym_solve(CovWWp, Y))
        assert np.array_equal(C, C11)
        alpha = orc._sym_solve(CovWWp, Y)
        assert np.max(np.abs(m - (Y - p.yNoise * alpha))) <= 1e-12 * np.max(np.abs(Y))


def test_filled_vector_is_the_scalar_restatement_bit_for_bit():
    c = cases.make_case(50, "UX", False, S=2, seed=9)
    for x in (0.6, -1.2):
        a = ot.expected_outcome(c, [x])
        b = ot.expected_outcome_vec(c, np.full((1, 50), x))
        for k in ("meanITE", "covITE", "meanSATE", "varSATE"):
            assert np.array_equal(a[k], b[k]), k


# ---- the structured forms against the dense blocks ------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("n", [24, 129])
def test_structured_curve_covariance_equals_the_dense_sum(n, shape):
    """P_ll' - v_l . v_l' with P_ll' = rho(a_l, a_l') beta against w' Cov(f(a_l), f(a_l') | Y) w summed over dense n x n blocks;
    the diagonal against the per-level variance w' (CovC22 + pred_noise I) w of expected_outcome; the plain form's mean and
    variance against conditional_sate of the dense blocks.  Bound: 1e-11 of the variance scale — the two sides differ by
    rounding only (the worst value is printed; DESIGN.md §16 records it)."""
    c = cases.make_case(n, shape, False, S=2, seed=3)
    A = ot.levels(c, 5)
    w = np.random.default_rng(n).standard_normal(n) / n
    exp = ot.expected_outcome(c, A)
    worst = 0.0
    for s in range(c["S"]):
        m, cv = ot.literal_outcome_curve(c, s, A, w)
        ms, cs = ot.structured_outcome_curve(c, s, A, w)
        scale = np.max(np.abs(np.diag(cs)))
        worst = max(worst, np.max(np.abs(cv[:, :, 0] - cs)) / scale, np.max(np.abs(m[:, 0] - ms)) / np.max(np.abs(ms)))
        assert np.max(np.abs(m[:, 0] - ms)) <= 1e-11 * np.max(np.abs(ms))
        assert np.max(np.abs(cv[:, :, 0] - cs)) <= 1e-11 * scale
        assert np.array_equal(cs, cs.T)
        for l, a in enumerate(A):
            var_l = float(w @ exp["covITE"][s, l] @ w)
            assert abs(cs[l, l] - var_l) <= 1e-11 * scale
            assert abs(ms[l] - float(w @ exp["meanITE"][:, s, l])) <= 1e-11 * np.max(np.abs(ms))
            pm, pv = ot.structured_outcome_average(c, s, a)
            worst = max(worst, abs(pv - exp["varSATE"][s, l]) / exp["varSATE"][s, l])
            assert abs(pm - exp["meanSATE"][s, l]) <= 1e-11 * abs(exp["meanSATE"][s, l])
            assert abs(pv - exp["varSATE"][s, l]) <= 1e-11 * exp["varSATE"][s, l]
    print(f"n={n} {shape}: worst structured - dense, relative to the variance scale: {worst:.3e}")


@pytest.mark.parametrize("shape,bt", [("UX", False), ("T", False), ("UX", True)])
def test_structured_vector_level_equals_the_dense_blocks(shape, bt):
    c = cases.make_case(129, shape, bt, S=2, seed=4)
    D = np.vstack([vr.policy(c, 2, seed=1), vr.mixed(c, seed=2)[0][None, :]])
    exp = ot.expected_outcome_vec(c, D)
    for s in range(2):
        for l in range(D.shape[0]):
            mi, m, v = ot.structured_outcome_vec(c, s, D[l])
            assert np.max(np.abs(mi - exp["meanITE"][:, s, l])) <= 1e-11 * np.max(np.abs(mi))
            assert abs(m - exp["meanSATE"][s, l]) <= 1e-11 * abs(exp["meanSATE"][s, l]) + 1e-13
            assert abs(v - exp["varSATE"][s, l]) <= 1e-11 * exp["varSATE"][s, l]


def test_outcome_covariance_without_features_is_semi_definite_to_rounding():
    """Shape "T": B is constant, so CovC22 = B - D A^-1 D' has rank one up to rounding and its smallest eigenvalue is a
    rounding-level number of either sign — the draws need the robust factorisation (and get the pred_noise jitter first)."""
    c = cases.make_case(129, "T", False, S=2, seed=3)
    exp = ot.expected_outcome(c, [0.4])
    for s in range(2):
        ev = np.linalg.eigvalsh(exp["covITE"][s, 0] - PN * np.eye(129))
        assert abs(ev[0]) <= 1e-11 * ev[-1]


def test_draw_cases_have_a_covariance_that_is_positive_to_rounding():
    """The condition of the GPU draw cases: the restatement's jitter-free covariance has smallest eigenvalue >= -1e-12 yScale."""
    for n, shape, seed, L in ot.DRAW_CASES:
        c = cases.make_case(n, shape, False, S=2, seed=seed)
        exp = ot.expected_outcome(c, ot.levels(c, L), pred_noise=0.0)
        for s in range(2):
            for l in range(L):
                ev = np.linalg.eigvalsh(exp["covITE"][s, l])
                print(f"n={n} {shape} s={s} l={l}: smallest eigenvalue {ev[0]:.3e}, largest {ev[-1]:.3e}, yScale {c['yScale'][s]:.3g}")
                assert ev[0] >= -1e-12 * c["yScale"][s]


def test_levels_helper():
    for bt in (False, True):
        c = cases.make_case(50, "UX", bt, S=1, seed=3)
        for L in (1, 5, 40, 130):
            A = ot.levels(c, L)
            assert A.shape == (L,) and np.all(np.isfinite(A))
    assert list(ot.levels(cases.make_case(50, "UX", True, S=1, seed=3), 3)) == [0.0, 1.0, 0.5]


# ---- the Python mirror: the keyword and its refusals, before any device call ----------------------------------------
def test_outcome_is_a_keyword_of_every_estimation_entry_point():
    import causalgpslc_jl_amd as gp
    for fn in (gp.predict, gp.ITEDistributions, gp.SATEDistributions, gp.ITEsamples, gp.sampleITE, gp.sampleSATE,
               gp.effectCurve, gp.sampleEffectCurve, gp.predictCounterfactualEffects):
        par = inspect.signature(fn).parameters
        assert "outcome" in par and par["outcome"].default is False, fn.__name__


def test_outcome_refusals_come_before_any_device_call():
    import causalgpslc_jl_amd as gp
    c = cases.make_case(12, "UX", False, S=2, seed=1)
    g = cases.gpslc_object(gp, c)
    D = np.stack([c["T"] + 0.5, c["T"]])
    w = np.full(12, 1.0 / 12)
    every = ((gp.predict, ([0.6, 0.2],)), (gp.SATEDistributions, (0.6,)), (gp.ITEDistributions, (0.6,)),
             (gp.ITEsamples, (0.6, 2)), (gp.sampleITE, (0.6,)), (gp.sampleSATE, (0.6,)), (gp.effectCurve, ([0.6, 0.2],)),
             (gp.sampleEffectCurve, ([0.6, 0.2],)))
    for fn, args in every:
        with pytest.raises(ValueError, match="difference of two outcomes"):
            fn(g, *args, outcome=True, baseline=0.0)
        with pytest.raises(ValueError, match="slope"):
            fn(g, *args, outcome=True, slope=True)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, D, outcome=True, weights=w)
    for fn in (gp.SATEDistributions, gp.sampleSATE):
        with pytest.raises(ValueError, match="scalar levels"):
            fn(g, c["T"] + 0.5, outcome=True, weights=w)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.effectCurve(g, D, outcome=True)
    for fn, args in ((gp.predict, ([0.6, 0.2],)), (gp.predict, (D,)), (gp.effectCurve, ([0.6, 0.2],)),
                     (gp.sampleEffectCurve, ([0.6, 0.2],)), (gp.predictCounterfactualEffects, (2,))):
        with pytest.raises(ValueError, match="devices"):
            fn(g, *args, outcome=True, devices=[0])
    assert g._ctx is None                                    # nothing above reached the device


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_header_and_both_binding_tables_name_the_outcome_symbols():
    from causalgpslc_jl_amd import _lib
    hdr = set(_lib.header_symbols())
    julia = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "julia", "GPSLCHip.jl")).read()
    for name in SYMBOLS:
        assert name in hdr and name in _lib.SIGNATURES
        assert re.search(r"ccall\(\(:" + name + r",\s*lib\)", julia), name
    # the twins' signatures, position for position
    assert _lib.SIGNATURES["gpslc_predict_outcome"] == _lib.SIGNATURES["gpslc_predict_slope"]
    assert _lib.SIGNATURES["gpslc_predict_outcome_vec"] == _lib.SIGNATURES["gpslc_predict_vec"]
    assert _lib.SIGNATURES["gpslc_ite_distributions_outcome"] == _lib.SIGNATURES["gpslc_ite_distributions_slope"]
    assert _lib.SIGNATURES["gpslc_ite_distributions_outcome_vec"] == _lib.SIGNATURES["gpslc_ite_distributions_vec"]
    txt = open(_lib.HEADER_PATH).read()
    assert "mu_i(a) = f_i(a)" in txt and "CovC22" in txt and "value of the treatment policy".upper() in txt.upper()
    for kw in ("outcome::Bool=false",):
        assert julia.count(kw) >= 7
