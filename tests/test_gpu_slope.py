"""Marginal effects — the slope d f_i(t) / dt at a scalar level (gpslc_predict_slope, gpslc_ite_distributions_slope and the Python
mirror's `slope=True`) — against the dense restatement in tests/slope_restatement.py, and against the library's own contrasts
where the central difference ties the two estimands together.

Bounds: those of test_gpu_contrast._check (the 1e-6 bounds of SURVEY §8d, then tight = 1e-9) with the variance's absolute term
scaled to this estimand: the prior variance of a slope is 2 yScale / tyLS^2 where that of a level is yScale.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import curve_restatement as cu
import gpslc_oracle as orc
import slope_restatement as sr
import weighted_restatement as wr

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
CONT = sorted(cases.SHAPES)


def _vscale(case):
    """The prior variance of the slope per posterior sample: what yScale is to an ordinary level."""
    return 2.0 * case["yScale"] / case["tyLS"] ** 2


def _check(exp, ms, vs, mi, case, samples=None, tight=1e-9):
    yS = _vscale(case)
    L = ms.shape[1]
    for s in (range(case["S"]) if samples is None else samples):
        for l in range(L):
            rm, rv = exp["meanSATE"][s, l], exp["varSATE"][s, l]
            ref = exp["meanITE"][:, s, l]
            print(f"s={s} l={l} mean {abs(ms[s, l] - rm):.3e} of {abs(rm):.3e}  var {abs(vs[s, l] - rv):.3e} of "
                  f"{abs(rv):.3e} (scale {yS[s]:.3g})  MeanITE {np.max(np.abs(mi[:, s, l] - ref)):.3e} of {np.max(np.abs(ref)):.3e}")
            assert abs(ms[s, l] - rm) <= 1e-6 * abs(rm) + 1e-12, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= 1e-6 * abs(rv) + 1e-9 * yS[s], (s, l, vs[s, l], rv)
            assert np.max(np.abs(mi[:, s, l] - ref)) <= 1e-6 * np.max(np.abs(ref)) + 1e-12, (s, l)
            assert abs(ms[s, l] - rm) <= tight * abs(rm) + 1e-13, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= tight * abs(rv) + 1e-12 * yS[s], (s, l, vs[s, l], rv)
            assert np.max(np.abs(mi[:, s, l] - ref)) <= tight * np.max(np.abs(ref)) + 1e-13, (s, l)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- 1. predict(..., slope=True) against the restatement ------------------------------------------------------------
@pytest.mark.parametrize("shape", CONT)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("L", [1, 5, 40])
def test_predict_slope_against_restatement(gp, n, L, shape):
    c = cases.make_case(n, shape, False, S=2, seed=31 + L + n)
    A = sr.levels(c, L)
    exp = sr.expected_slope(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, slope=True)
    _check(exp, ms, vs, mi, c)


def test_predict_slope_binary_treatment_through_the_c_entry_point(gp):
    """The slope of the response surface is defined for a binary treatment too (the surface is a GP over the real line), and
    binary_t switches the Gram kernel: the plain form of gpslc_predict_slope itself, G = 0 and no weights."""
    n, S, L = 129, 2, 3
    c = cases.make_case(n, "UX", True, S=S, seed=32)
    A = np.ascontiguousarray(sr.levels(c, L))
    exp = sr.expected_slope(c, A, want_cov=False)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    ms, vs, mi = np.empty((S, L), order="F"), np.empty((S, L), order="F"), np.empty((n, S, L), order="F")
    st = ctx.lib.gpslc_predict_slope(ctx.h, S, *g._params(), L, _p(A), 0, None, PN, 0, 0, None, _p(ms), _p(vs), None, _p(mi), None)
    assert st == 0
    _check(exp, ms, vs, mi, c)


# ---- 2. where the layouts switch ------------------------------------------------------------------------------------
def test_predict_slope_two_augmented_tile_rows(gp):
    """L = 130: 131 right-hand sides, two augmented tile rows."""
    c = cases.make_case(24, "UX", False, S=2, seed=33)
    A = sr.levels(c, 130)
    exp = sr.expected_slope(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, slope=True)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("L", [15, 16, 31, 32, 126, 127])
def test_predict_slope_where_the_right_hand_side_layout_switches(gp, L):
    """16 / 17, 32 / 33 and 127 / 128 right-hand sides (Y + L levels): 16 live rows, 32 live rows, a full augmented tile row,
    and the last count before a second one — on two tiles per side."""
    c = cases.make_case(200, "UX", False, S=2, seed=35 + L)
    A = sr.levels(c, L)
    exp = sr.expected_slope(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, slope=True)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("L", [3, 40])
def test_predict_slope_persistent_task_launch(gp, L):
    """The persistent launch forced down to one matrix (gpslc_set_task_schedule) really runs for a slope call, and gives the
    per-column schedule's outputs bit for bit; both against the restatement."""
    c = cases.make_case(520, "UX", False, S=5, seed=41)
    A = sr.levels(c, L)
    out = []
    for tiles in (32, 0):
        g = cases.gpslc_object(gp, c)
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)      # HIP-event records: which schedule really ran
        g._ctx.set_data(g.X, g.T, g.Y)
        g.ctx().set_task_schedule(2, tiles, 1, 0)
        g.ctx().profile_reset()
        out.append(gp.predict(g, A, want_mean_ite=True, slope=True))
        assert (g.ctx().profile_get(4)[0] > 0) == (tiles > 0)
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    chk = [0, 4]
    exp = sr.expected_slope(c, A, samples=chk, want_cov=False)
    _check(exp, *out[0], c, samples=chk)


# ---- 3. the weighted form and the joint covariance ------------------------------------------------------------------
def _weights_for(c, G):
    """(what the caller passes, the float weights it means): G = 1 a Bool mask of the upper half of T; G = 3 the mask, a zero
    column and random signed weights."""
    n, T = c["n"], c["T"]
    mask = T > np.median(T)
    if G == 1:
        return mask, (mask / mask.sum())[None, :]
    Wf = np.stack([mask / mask.sum(), np.zeros(n), np.random.default_rng(7).standard_normal(n) / n])
    return Wf, Wf


@pytest.mark.parametrize("n,shape", [(24, "UX"), (129, "T"), (129, "UX"), (200, "X")])
@pytest.mark.parametrize("G", [1, 3])
def test_weighted_slope_and_its_joint_covariance_against_restatement(gp, n, shape, G):
    c = cases.make_case(n, shape, False, S=2, seed=201 + n + G)
    L = 4
    A = sr.levels(c, L)
    given, W = _weights_for(c, G)
    exp = sr.expected_slope_curve(c, A, W)
    g = cases.gpslc_object(gp, c)
    m, cov = gp.effectCurve(g, A, weights=given, slope=True)
    mp, vp, _ = gp.predict(g, A, weights=given, slope=True)
    if G == 1:
        assert m.shape == (2, L) and cov.shape == (2, L, L) and mp.shape == (2, L)
        m, cov, mp, vp = m[:, :, None], cov[:, :, :, None], mp[:, :, None], vp[:, :, None]
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1, 3)))               # exactly symmetric
    for l in range(L):
        assert np.array_equal(cov[:, l, l, :], vp[:, l, :])                    # the diagonal is varW to the bits
    assert np.array_equal(m, mp)
    vsc = _vscale(c)
    worst_m = worst_c = 0.0
    for s in range(2):
        for k in range(W.shape[0]):
            for l in range(L):
                rm = exp["mean"][s, l, k]
                bm, _, tm, _ = wr.bounds(rm, 0.0, W[k], vsc[s])
                em = abs(m[s, l, k] - rm)
                assert em <= bm and em <= tm, (s, l, k, m[s, l, k], rm)
                worst_m = max(worst_m, em / tm) if tm > 0 else worst_m
                for lp in range(L):
                    rc = exp["cov"][s, l, lp, k]
                    _, bc, _, tc = wr.bounds(0.0, rc, W[k], vsc[s])
                    ec = abs(cov[s, l, lp, k] - rc)
                    assert ec <= bc and ec <= tc, (s, l, lp, k, cov[s, l, lp, k], rc)
                    worst_c = max(worst_c, ec / tc) if tc > 0 else worst_c
    print(f"worst error / tight bound: mean {worst_m:.3e} cov {worst_c:.3e}")
    if G == 3:              # a zero weight column gives an all-0.0 block and zero means
        assert np.all(cov[:, :, :, 1] == 0.0) and np.all(m[:, :, 1] == 0.0)
    # curveSamples takes the blocks as they are: against the pivoted-Cholesky reference on the same blocks.  The two sides run
    # the same algorithm in fp64 on the same input, so they differ by eps * cond(block); the levels are distinct: cond < 1e6
    spp = 3
    z = np.random.default_rng(5).standard_normal((L, spp, 2, W.shape[0]))
    dr = gp.curveSamples(m, cov, spp, z=z)
    ref = cu.curve_samples(m, cov, spp, z)
    for s in range(2):
        for k in range(W.shape[0]):
            if not np.any(W[k]):
                continue
            assert np.linalg.cond(cov[s, :, :, k]) < 1e6
    assert np.all(np.isfinite(dr)) and np.max(np.abs(dr - ref)) <= 1e-9 * np.max(np.abs(ref))


def test_other_outputs_do_not_depend_on_the_joint_covariance(gp):
    """meanW, varW, MeanITE and the draws are bit-identical with and without covW; the plain form's MeanITE and draws are the
    weighted form's."""
    c = cases.make_case(200, "UX", False, S=3, seed=231)
    A = sr.levels(c, 4)
    W = wr.weight_set(c)
    g = cases.gpslc_object(gp, c)
    kw = dict(weights=W, want_mean_ite=True, spp=4, seed=9, want_draws=True, slope=True)
    (mw, vw, cw, mi, dr), _ = gp.api._predict_curve(g, A, **kw)
    (mw2, vw2, none, mi2, dr2), _ = gp.api._predict_curve(g, A, want_cov=False, **kw)
    assert none is None and cw is not None
    for a, b in zip((mw, vw, mi, dr), (mw2, vw2, mi2, dr2)):
        assert np.array_equal(a, b)
    ref = gp.predict(g, A, **kw)
    for a, b in zip((mw, vw, mi, dr), ref):
        assert np.array_equal(a, b)
    plain = gp.predict(g, A, want_mean_ite=True, spp=4, seed=9, want_draws=True, slope=True)
    assert np.array_equal(plain[2], mi) and np.array_equal(plain[3], dr)
    # w = 1/n through the weighted form is the plain form's average up to the order of summation
    assert np.allclose(mw[:, :, 0], plain[0], rtol=1e-9, atol=1e-13)
    assert np.allclose(vw[:, :, 0], plain[1], rtol=1e-9, atol=1e-12 * np.max(_vscale(c)))
    # effectCurve without weights is w = 1/n
    m0, c0 = gp.effectCurve(g, A, slope=True)
    assert np.array_equal(m0, mw[:, :, 0]) and np.array_equal(c0, cw[:, :, :, 0])


# ---- 4. ITEDistributions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(129, "UX"), (129, "T"), (200, "UX"), (200, "X")])
def test_ite_distributions_slope_against_restatement(gp, n, shape):
    c = cases.make_case(n, shape, False, S=2, seed=51 + n)
    a = 0.6
    M, CV = gp.ITEDistributions(cases.gpslc_object(gp, c), a, slope=True)
    Mr, CVr = sr.ite_distributions_slope(cases.samples_of(c), c["X"], c["T"], c["Y"], a)
    vsc = _vscale(c)
    for s in range(c["S"]):
        em, ec = np.max(np.abs(M[s] - Mr[s])), np.max(np.abs(CV[s] - CVr[s]))
        print(f"s={s} MeanITEs {em:.3e} of {np.max(np.abs(Mr[s])):.3e}  CovITEs {ec:.3e} (scale {vsc[s]:.3g})")
        assert em <= 1e-9 * np.max(np.abs(Mr[s])) + 1e-13
        assert ec <= 1e-9 * vsc[s]
        assert np.array_equal(CV[s], CV[s].T)


# ---- 5. draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [PN, 1e-3])
@pytest.mark.parametrize("n,L,shape", [(129, 1, "UX"), (200, 3, "UX"), (150, 2, "T")])
def test_draws_with_caller_normals_against_restatement(gp, n, L, shape, pn):
    c = cases.make_case(n, shape, False, S=2, seed=61)
    A = sr.levels(c, L)
    exp = sr.expected_slope(c, A, pred_noise=pn)
    spp = 3
    z = np.random.default_rng(62).standard_normal((n, spp, c["S"], L))
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn))
    _, _, mi, dr = gp.predict(g, A, want_mean_ite=True, spp=spp, z=z, want_draws=True, slope=True)
    for s in range(c["S"]):
        for l in range(L):
            Cm = exp["covITE"][s, l]
            Lc = np.linalg.cholesky(Cm)
            ref = exp["meanITE"][:, s, l][:, None] + Lc @ z[:, :, s, l]
            ev = np.linalg.eigvalsh(Cm)
            bound, tight, cond = cases.draw_bounds(ev[0], ev[-1], np.linalg.norm(z[:, :, s, l]), np.linalg.norm(ref))
            err = np.linalg.norm(dr[l, :, spp * s:spp * s + spp] - ref)
            print(f"s={s} l={l} cond {cond:.3e} error {err:.3e} bound {bound:.3e} tight {tight}")
            assert err <= bound, (s, l)
            assert tight is None or err <= tight, (s, l, cond)


def test_seeded_draws_are_reproducible_and_chunking_independent(gp):
    c = cases.make_case(200, "UX", False, S=6, seed=71)
    A = sr.levels(c, 3)
    g = cases.gpslc_object(gp, c)
    kw = dict(want_mean_ite=True, spp=5, want_draws=True, slope=True)
    first = gp.predict(g, A, seed=9, **kw)
    again = gp.predict(g, A, seed=9, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    other = gp.predict(g, A, seed=10, **kw)
    assert np.array_equal(first[2], other[2]) and not np.array_equal(first[3], other[3])
    g4 = cases.gpslc_object(gp, c)
    g4.ctx().set_tuning(max_batch=4)
    chunked = gp.predict(g4, A, seed=9, **kw)
    for a, b in zip(first, chunked):
        assert np.array_equal(a, b)
    # sampleITE / sampleSATE take the keyword
    ite = gp.sampleITE(g, A[0], samplesPerPosterior=5, seed=9, slope=True)
    assert np.array_equal(ite, np.asfortranarray(gp.predict(g, [A[0]], seed=9, **kw)[3][0]))
    zs = np.random.default_rng(82).standard_normal(c["S"] * 4)
    got = gp.sampleSATE(g, A[0], samplesPerPosterior=4, z=zs, slope=True)
    assert np.allclose(got, orc.sate_samples(first[0][:, 0], first[1][:, 0], 4, zs), rtol=1e-12, atol=0.0)


# ---- 6. GPU against GPU: the central difference of the library's contrasts ------------------------------------------
@pytest.mark.parametrize("n,shape,seed,a", sr.FD_CASES)
def test_central_difference_of_contrasts_agrees_with_the_slope(gp, n, shape, seed, a):
    """predict(g, a + h, baseline=a - h) / (2h) against the slope at h = 1e-3, a check that does not rest on the restatement.
    The bound is twice the truncation error of the central difference measured on the CPU for the same cases
    (slope_restatement.FD_MEASURED; tests/test_slope.py keeps the record honest): per case, relative to the slope's own size,
        (129, "UX")  MeanITE 4.675e-06  mean 8.044e-06  variance 1.450e-05
        (200, "X")   MeanITE 8.243e-07  mean 3.306e-07  variance 3.552e-06
        (129, "T")   MeanITE 5.799e-04  mean 5.799e-04  variance 8.101e-06
        (24, "U")    MeanITE 2.550e-06  mean 2.425e-06  variance 9.672e-06
    The contrast's own rounding at levels 2h apart (r^a - r^b and 1 - rho cancel: about 1e-13 and 3e-11 relative) is far below
    these.  The pred_noise jitter is not part of either estimand's curvature: it is taken off both variances first."""
    h = sr.FD_H
    e_ite, _, e_mean, e_var = sr.FD_MEASURED[(n, shape)]
    c = cases.make_case(n, shape, False, S=2, seed=seed)
    g = cases.gpslc_object(gp, c)
    ms, vs, mi = gp.predict(g, [a], want_mean_ite=True, slope=True)
    mc, vc, mic = gp.predict(g, [a + h], want_mean_ite=True, baseline=a - h)
    jit = PN / n
    for s in range(2):
        d_ite = np.max(np.abs(mic[:, s, 0] / (2 * h) - mi[:, s, 0])) / np.max(np.abs(mi[:, s, 0]))
        d_mean = abs(mc[s, 0] / (2 * h) - ms[s, 0]) / abs(ms[s, 0])
        v_s, v_c = vs[s, 0] - jit, (vc[s, 0] - jit) / (4 * h * h)
        d_var = abs(v_c - v_s) / abs(v_s)
        print(f"s={s} MeanITE {d_ite:.3e} (bound {2 * e_ite:.3e})  mean {d_mean:.3e} ({2 * e_mean:.3e})  var {d_var:.3e} ({2 * e_var:.3e})")
        assert d_ite <= 2 * e_ite and d_mean <= 2 * e_mean and d_var <= 2 * e_var


# ---- 7. error paths -------------------------------------------------------------------------------------------------
def test_fp32_context_refuses_slopes(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=91)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.SATEDistributions(g, 0.6, slope=True)
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.ITEDistributions(g, 0.6, slope=True)
    assert ei.value.status == -1007
    with pytest.raises(gp.GPSLCError) as ei:
        gp.effectCurve(g, [0.6, 0.1], slope=True)
    assert ei.value.status == -1007
    gp.SATEDistributions(g, 0.6)               # the ordinary level of the same context keeps working


def test_c_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=92)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    lib = ctx.lib
    n, S = 24, 2
    ms, vs = np.empty((S, 2), order="F"), np.empty((S, 2), order="F")
    cw = np.empty((S, 2, 2, 1), order="F")
    ok = np.array([0.6, 0.1])
    w = np.full(n, 1.0 / n)

    def call(doT=ok, G=0, W=None, spp=0, ms_=ms, vs_=vs, cov=None, dr=None, L=2):
        return lib.gpslc_predict_slope(ctx.h, S, *g._params(), L, _p(doT), G, _p(W), PN, spp, 0, None, _p(ms_), _p(vs_),
                                       _p(cov), None, _p(dr))

    for bad in (np.array([0.6, np.nan]), np.array([np.inf, 0.1]), None):
        assert call(doT=bad) == -10
        assert "argument #10" in lib.gpslc_last_error(ctx.h).decode()
    assert call(L=0) == -9
    assert call(G=-1) == -11 and "argument #11" in lib.gpslc_last_error(ctx.h).decode()
    assert call(G=0, W=w) == -11
    assert call(G=1, W=None) == -12 and "argument #12" in lib.gpslc_last_error(ctx.h).decode()
    wbad = w.copy()
    wbad[3] = np.nan
    assert call(G=1, W=wbad) == -12
    dr = np.empty((2, n, S))
    assert call(dr=dr) == -14 and "argument #14" in lib.gpslc_last_error(ctx.h).decode()
    assert call(G=1, W=w, dr=dr) == -14
    assert call(cov=cw) == -19 and "argument #19" in lib.gpslc_last_error(ctx.h).decode()
    M = np.empty((S, n))
    assert lib.gpslc_ite_distributions_slope(ctx.h, S, *g._params(), float("nan"), PN, _p(M), None) == -9
    assert "argument #9" in lib.gpslc_last_error(ctx.h).decode()
    assert lib.gpslc_ite_distributions_slope(ctx.h, S, *g._params(), float("inf"), PN, _p(M), None) == -9
    assert lib.gpslc_ite_distributions_slope(ctx.h, S, *g._params(), 0.6, PN, _p(M), None) == 0
    # the good calls: plain, and weighted with the covariance
    assert call() == 0
    mw, vw = np.empty((S, 2, 1), order="F"), np.empty((S, 2, 1), order="F")
    assert call(G=1, W=w, ms_=mw, vs_=vw, cov=cw) == 0
    assert np.allclose(mw[:, :, 0], ms, rtol=1e-9, atol=1e-13) and np.array_equal(cw[:, 0, 0, 0], vw[:, 0, 0])
    assert np.all(np.isfinite(M))
