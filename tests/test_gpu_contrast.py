"""Contrasts between two intervention levels (gpslc_predict_contrast, gpslc_ite_distributions_contrast and the Python mirror's
`baseline=`) against the dense restatement in tests/contrast_restatement.py, and against the ordinary levels where an identity
ties the two estimands together."""
import ctypes as C

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import gpslc_oracle as orc

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


def _check(exp, ms, vs, mi, case, samples=None, tight=1e-9):
    """The bounds test_gpu_estimation._check_against applies to the scalar path, then what fp64 delivers."""
    yS = case["yScale"]
    L = ms.shape[1]
    for s in (range(case["S"]) if samples is None else samples):
        for l in range(L):
            rm, rv = exp["meanSATE"][s, l], exp["varSATE"][s, l]
            ref = exp["meanITE"][:, s, l]
            print(f"s={s} l={l} meanSATE {abs(ms[s, l] - rm):.3e} of {abs(rm):.3e}  varSATE {abs(vs[s, l] - rv):.3e} of "
                  f"{abs(rv):.3e} (yScale {yS[s]:.3g})  MeanITE {np.max(np.abs(mi[:, s, l] - ref)):.3e} of {np.max(np.abs(ref)):.3e}")
            assert abs(ms[s, l] - rm) <= 1e-6 * abs(rm) + 1e-12, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= 1e-6 * abs(rv) + 1e-9 * yS[s], (s, l, vs[s, l], rv)
            assert np.max(np.abs(mi[:, s, l] - ref)) <= 1e-6 * np.max(np.abs(ref)) + 1e-12, (s, l)
            assert abs(ms[s, l] - rm) <= tight * abs(rm) + 1e-13, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= tight * abs(rv) + 1e-12 * yS[s], (s, l, vs[s, l], rv)
            assert np.max(np.abs(mi[:, s, l] - ref)) <= tight * np.max(np.abs(ref)) + 1e-13, (s, l)


# ---- 1. predict(..., baseline=) against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("L", [1, 5, 40])
def test_predict_contrast_against_restatement(gp, n, L, shape, bt):
    c = cases.make_case(n, shape, bt, S=2, seed=31 + L + n)
    A, B = cr.pairs(c, L)
    exp = cr.expected_contrast(c, A, B, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, baseline=B)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("bt", [False, True])
def test_predict_contrast_two_augmented_tile_rows(gp, bt):
    """L = 130: 131 right-hand sides, two augmented tile rows."""
    c = cases.make_case(24, "UX", bt, S=2, seed=33)
    A, B = cr.pairs(c, 130)
    exp = cr.expected_contrast(c, A, B, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, baseline=B)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("L", [15, 16, 31, 32, 126, 127])
def test_predict_contrast_where_the_right_hand_side_layout_switches(gp, L):
    """16 / 17, 32 / 33 and 127 / 128 right-hand sides (Y + L levels): 16 live rows, 32 live rows, a full augmented tile row,
    and the last count before a second one — on two tiles per side."""
    c = cases.make_case(200, "UX", False, S=2, seed=35 + L)
    A, B = cr.pairs(c, L)
    exp = cr.expected_contrast(c, A, B, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, baseline=B)
    _check(exp, ms, vs, mi, c)


def test_scalar_baseline_is_every_levels_baseline(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=37)
    g = cases.gpslc_object(gp, c)
    A = np.array([0.6, -0.9, 1.2])
    a = gp.predict(g, A, want_mean_ite=True, baseline=0.1)
    b = gp.predict(g, A, want_mean_ite=True, baseline=[0.1, 0.1, 0.1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- 2. exact zeros -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
def test_exact_zeros_when_both_levels_are_the_same(gp, shape, bt):
    n = 150
    c = cases.make_case(n, shape, bt, S=2, seed=21)
    g = cases.gpslc_object(gp, c)
    a = 1.0 if bt else 0.37
    for L in (1, 6):            # the VALU and the MFMA MeanITE kernel
        A = np.full(L, a)
        other = 0.0 if bt else -0.8
        A[L // 2:L // 2 + (L > 1)] = other            # L = 6: one real contrast among the equal pairs
        ms, vs, mi = gp.predict(g, A, want_mean_ite=True, baseline=a)
        same = A == a
        assert np.all(ms[:, same] == 0.0)
        assert np.all(vs[:, same] == (n * PN) / (n * n))
        assert np.all(mi[:, :, same] == 0.0)
        if L > 1:
            assert np.all(ms[:, ~same] != 0.0) and np.all(vs[:, ~same] != (n * PN) / (n * n)) and np.any(mi[:, :, ~same] != 0.0)
    M, CV = gp.ITEDistributions(g, a, baseline=a)
    assert np.all(M == 0.0)
    for s in range(c["S"]):
        assert np.array_equal(CV[s], PN * np.eye(n))
    ms, vs = gp.SATEDistributions(g, a, baseline=a)
    assert np.all(ms == 0.0) and np.all(vs == (n * PN) / (n * n))


# ---- 3. the binary-treatment identity, GPU against GPU --------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("n", [129, 400])
def test_binary_contrast_against_the_ordinary_levels(gp, n, shape):
    """f_i(1) - f_i(0) is MeanITE_i(1) where T_i == 0 and -MeanITE_i(0) where T_i == 1: a check on the existing predict outputs
    that does not rest on the restatement.  (0, 1) is the negated pair; both in one call, L = 2."""
    c = cases.make_case(n, shape, True, S=3, seed=43 + n)
    g = cases.gpslc_object(gp, c)
    T = c["T"]
    ms01, _, mi01 = gp.predict(g, [0.0, 1.0], want_mean_ite=True)
    ms, vs, mi = gp.predict(g, [1.0, 0.0], want_mean_ite=True, baseline=[0.0, 1.0])
    for s in range(c["S"]):
        scale = max(np.max(np.abs(mi01[:, s, 0])), np.max(np.abs(mi01[:, s, 1])))
        e0 = np.max(np.abs(mi[T == 0, s, 0] - mi01[T == 0, s, 1]))
        e1 = np.max(np.abs(mi[T == 1, s, 0] + mi01[T == 1, s, 0]))
        es = abs(ms[s, 0] - (ms01[s, 1] - ms01[s, 0]))
        print(f"s={s} untreated {e0:.3e} treated {e1:.3e} SATE {es:.3e} of {scale:.3e}")
        assert e0 <= 1e-9 * scale and e1 <= 1e-9 * scale
        assert es <= 1e-9 * scale
        assert np.max(np.abs(mi[:, s, 1] + mi[:, s, 0])) <= 1e-12 * scale
        assert abs(vs[s, 1] - vs[s, 0]) <= 1e-9 * vs[s, 0]


# ---- 4. ITEDistributions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,bt", [(129, "UX", False), (129, "T", True), (200, "UX", True), (200, "X", False)])
def test_ite_distributions_contrast_against_restatement(gp, n, shape, bt):
    c = cases.make_case(n, shape, bt, S=2, seed=51 + n)
    a, b = (1.0, 0.0) if bt else (0.6, -0.4)
    M, CV = gp.ITEDistributions(cases.gpslc_object(gp, c), a, baseline=b)
    Mr, CVr = cr.ite_distributions_contrast(cases.samples_of(c), c["X"], c["T"], c["Y"], a, b)
    for s in range(c["S"]):
        em, ec = np.max(np.abs(M[s] - Mr[s])), np.max(np.abs(CV[s] - CVr[s]))
        print(f"s={s} MeanITEs {em:.3e} of {np.max(np.abs(Mr[s])):.3e}  CovITEs {ec:.3e} (yScale {c['yScale'][s]:.3g})")
        assert em <= 1e-9 * np.max(np.abs(Mr[s])) + 1e-13
        assert ec <= 1e-9 * c["yScale"][s]
        assert np.array_equal(CV[s], CV[s].T)


# ---- 5. draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [PN, 1e-3])
@pytest.mark.parametrize("n,L,bt", [(129, 1, False), (200, 3, False), (150, 2, True)])
def test_draws_with_caller_normals_against_restatement(gp, n, L, bt, pn):
    c = cases.make_case(n, "UX", bt, S=2, seed=61)
    A, B = cr.pairs(c, L)
    exp = cr.expected_contrast(c, A, B, pred_noise=pn)
    spp = 3
    z = np.random.default_rng(62).standard_normal((n, spp, c["S"], L))
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn))
    _, _, mi, dr = gp.predict(g, A, want_mean_ite=True, spp=spp, z=z, want_draws=True, baseline=B)
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
    A, B = cr.pairs(c, 3)
    g = cases.gpslc_object(gp, c)
    first = gp.predict(g, A, want_mean_ite=True, spp=5, seed=9, want_draws=True, baseline=B)
    again = gp.predict(g, A, want_mean_ite=True, spp=5, seed=9, want_draws=True, baseline=B)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    other = gp.predict(g, A, want_mean_ite=True, spp=5, seed=10, want_draws=True, baseline=B)
    assert np.array_equal(first[2], other[2]) and not np.array_equal(first[3], other[3])
    g4 = cases.gpslc_object(gp, c)
    g4.ctx().set_tuning(max_batch=4)
    chunked = gp.predict(g4, A, want_mean_ite=True, spp=5, seed=9, want_draws=True, baseline=B)
    for a, b in zip(first, chunked):
        assert np.array_equal(a, b)


# ---- 6. the persistent task launch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 40])
def test_predict_contrast_persistent_task_launch(gp, L):
    """The persistent launch forced down to one matrix (gpslc_set_task_schedule) really runs for a contrast call, and gives
    the per-column schedule's outputs bit for bit; both against the restatement."""
    c = cases.make_case(520, "UX", False, S=5, seed=41)
    A, B = cr.pairs(c, L)
    out = []
    for tiles in (32, 0):
        g = cases.gpslc_object(gp, c)
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)      # HIP-event records: which schedule really ran
        g._ctx.set_data(g.X, g.T, g.Y)
        g.ctx().set_task_schedule(2, tiles, 1, 0)
        g.ctx().profile_reset()
        out.append(gp.predict(g, A, want_mean_ite=True, baseline=B))
        assert (g.ctx().profile_get(4)[0] > 0) == (tiles > 0)
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    chk = [0, 4]
    exp = cr.expected_contrast(c, A, B, samples=chk, want_cov=False)
    _check(exp, *out[0], c, samples=chk)


# ---- 7. public surface ----------------------------------------------------------------------------------------------
def test_sample_sate_and_ite_take_the_baseline(gp):
    n = 129
    c = cases.make_case(n, "UX", False, S=3, seed=81)
    g = cases.gpslc_object(gp, c)
    a, b = 0.6, -0.4
    exp = cr.expected_contrast(c, [a], [b])
    z = np.random.default_rng(82).standard_normal(c["S"] * 4)
    got = gp.sampleSATE(g, a, samplesPerPosterior=4, z=z, baseline=b)
    ref = orc.sate_samples(exp["meanSATE"][:, 0], exp["varSATE"][:, 0], 4, z)
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-12)
    plain = gp.sampleSATE(g, a, samplesPerPosterior=4, z=z)
    assert not np.allclose(got, plain, rtol=1e-3)
    zi = np.random.default_rng(83).standard_normal((n, c["S"] * 4))
    ite = gp.sampleITE(g, a, samplesPerPosterior=4, z=zi, baseline=b)
    M, CV = cr.ite_distributions_contrast(cases.samples_of(c), c["X"], c["T"], c["Y"], a, b)
    ref = orc.ite_samples(M, CV, 4, zi)
    for s in range(c["S"]):
        ev = np.linalg.eigvalsh(CV[s])
        cols = slice(4 * s, 4 * s + 4)
        bound, _, _ = cases.draw_bounds(ev[0], ev[-1], np.linalg.norm(zi[:, cols]), np.linalg.norm(ref[:, cols]))
        assert np.linalg.norm(ite[:, cols] - ref[:, cols]) <= bound, s
    m, v = gp.SATEDistributions(g, a, baseline=b)
    assert np.allclose(m, exp["meanSATE"][:, 0], rtol=1e-9, atol=1e-13)


def test_fp32_context_refuses_contrasts(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=91)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.SATEDistributions(g, 0.6, baseline=-0.4)
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.ITEDistributions(g, 0.6, baseline=-0.4)
    assert ei.value.status == -1007
    gp.SATEDistributions(g, 0.6)               # the ordinary level of the same context keeps working


def test_c_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=92)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    lib = ctx.lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, S = 24, 2
    ms, vs = np.empty((S, 2), order="F"), np.empty((S, 2), order="F")
    ok = np.array([0.6, 0.1])
    for bad in (np.array([0.6, np.nan]), np.array([np.inf, 0.1]), None):
        assert lib.gpslc_predict_contrast(ctx.h, S, *g._params(), 2, p(bad), p(ok), PN, 0, 0, None, p(ms), p(vs), None, None) == -10
        assert "argument #10" in lib.gpslc_last_error(ctx.h).decode()
        assert lib.gpslc_predict_contrast(ctx.h, S, *g._params(), 2, p(ok), p(bad), PN, 0, 0, None, p(ms), p(vs), None, None) == -11
        assert "argument #11" in lib.gpslc_last_error(ctx.h).decode()
    # L = 0 is rejected as gpslc_predict rejects it; draws without spp name spp's own position in this signature
    assert lib.gpslc_predict(ctx.h, S, *g._params(), 0, p(ok), PN, 0, 0, None, p(ms), p(vs), None, None) == -9
    assert lib.gpslc_predict_contrast(ctx.h, S, *g._params(), 0, p(ok), p(ok), PN, 0, 0, None, p(ms), p(vs), None, None) == -9
    dr = np.empty((2, n, S))
    assert lib.gpslc_predict_contrast(ctx.h, S, *g._params(), 2, p(ok), p(ok), PN, 0, 0, None, p(ms), p(vs), None, p(dr)) == -13
    M = np.empty((S, n))
    assert lib.gpslc_ite_distributions_contrast(ctx.h, S, *g._params(), float("nan"), 0.1, PN, p(M), None) == -9
    assert "argument #9" in lib.gpslc_last_error(ctx.h).decode()
    assert lib.gpslc_ite_distributions_contrast(ctx.h, S, *g._params(), 0.6, float("-inf"), PN, p(M), None) == -10
    assert "argument #10" in lib.gpslc_last_error(ctx.h).decode()
    assert lib.gpslc_ite_distributions_contrast(ctx.h, S, *g._params(), 0.6, 0.1, PN, p(M), None) == 0
    assert lib.gpslc_predict_contrast(ctx.h, S, *g._params(), 2, p(ok), p(ok[::-1].copy()), PN, 0, 0, None, p(ms), p(vs), None, None) == 0
    assert np.allclose(ms[:, 1], -ms[:, 0], rtol=1e-12, atol=0)
