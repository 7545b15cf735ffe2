"""Potential outcomes — the response surface f_i(a) itself at scalar levels (gpslc_predict_outcome,
gpslc_ite_distributions_outcome) and at per-individual levels (gpslc_predict_outcome_vec, gpslc_ite_distributions_outcome_vec),
and the Python mirror's `outcome=True` — against the dense restatement in tests/outcome_restatement.py, and against the library's
own ordinary levels, contrasts and likelihood blocks where an identity ties the estimands together.

Bounds: test_gpu_contrast._check's for scalar levels (the 1e-6 bounds of SURVEY §8d, then tight = 1e-9; the variance's absolute
term is scaled by yScale, which is the prior variance of an outcome level) and test_gpu_vector_intervention._check's for vector
levels.  No bound of this file is its own.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import curve_restatement as cu
import gpslc_oracle as orc
import outcome_restatement as ot
import vector_restatement as vr
import weighted_restatement as wr
from test_gpu_contrast import _check
from test_gpu_vector_intervention import _check as _check_vec

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
CONT = sorted(cases.SHAPES)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _forced_schedules(gp, c, run):
    """`run(g)` under the persistent task launch forced down to one matrix and under the per-column schedule: the two outputs,
    after checking with the HIP-event records which schedule really ran."""
    out = []
    for tiles in (32, 0):
        g = cases.gpslc_object(gp, c)
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)
        g._ctx.set_data(g.X, g.T, g.Y)
        g.ctx().set_task_schedule(2, tiles, 1, 0)
        g.ctx().profile_reset()
        out.append(run(g))
        assert (g.ctx().profile_get(4)[0] > 0) == (tiles > 0)
    return out


# ---- 1. predict(..., outcome=True) at scalar levels against the restatement -------------------------------------------
@pytest.mark.parametrize("shape", CONT)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("L", [1, 5, 40])
def test_predict_outcome_against_restatement(gp, n, L, shape):
    c = cases.make_case(n, shape, False, S=2, seed=31 + L + n)
    A = ot.levels(c, L)
    exp = ot.expected_outcome(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, outcome=True)
    _check(exp, ms, vs, mi, c)


def test_predict_outcome_binary_treatment_through_the_c_entry_point(gp):
    """E[Y(0)], E[Y(1)] and the level between them; binary_t switches the Gram kernel: the plain form of gpslc_predict_outcome
    itself, G = 0 and no weights."""
    n, S, L = 129, 2, 3
    c = cases.make_case(n, "UX", True, S=S, seed=32)
    A = np.ascontiguousarray(ot.levels(c, L))
    assert list(A) == [0.0, 1.0, 0.5]
    exp = ot.expected_outcome(c, A, want_cov=False)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    ms, vs, mi = np.empty((S, L), order="F"), np.empty((S, L), order="F"), np.empty((n, S, L), order="F")
    st = ctx.lib.gpslc_predict_outcome(ctx.h, S, *g._params(), L, _p(A), 0, None, PN, 0, 0, None, _p(ms), _p(vs), None, _p(mi), None)
    assert st == 0
    _check(exp, ms, vs, mi, c)


# ---- 2. where the layouts switch ------------------------------------------------------------------------------------
def test_predict_outcome_two_augmented_tile_rows(gp):
    """L = 130: 131 right-hand sides, two augmented tile rows."""
    c = cases.make_case(24, "UX", False, S=2, seed=33)
    A = ot.levels(c, 130)
    exp = ot.expected_outcome(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, outcome=True)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("L", [15, 16, 31, 32, 126, 127])
def test_predict_outcome_where_the_right_hand_side_layout_switches(gp, L):
    """16 / 17, 32 / 33 and 127 / 128 right-hand sides (Y + L levels): 16 live rows, 32 live rows, a full augmented tile row,
    and the last count before a second one — on two tiles per side."""
    c = cases.make_case(200, "UX", False, S=2, seed=35 + L)
    A = ot.levels(c, L)
    exp = ot.expected_outcome(c, A, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), A, want_mean_ite=True, outcome=True)
    _check(exp, ms, vs, mi, c)


@pytest.mark.parametrize("L", [3, 40])
def test_predict_outcome_persistent_task_launch(gp, L):
    """The persistent launch forced down to one matrix (gpslc_set_task_schedule) really runs for an outcome call, and gives the
    per-column schedule's outputs bit for bit; both against the restatement."""
    c = cases.make_case(520, "UX", False, S=5, seed=41)
    A = ot.levels(c, L)
    out = _forced_schedules(gp, c, lambda g: gp.predict(g, A, want_mean_ite=True, outcome=True))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    chk = [0, 4]
    exp = ot.expected_outcome(c, A, samples=chk, want_cov=False)
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
def test_weighted_outcome_and_its_joint_covariance_against_restatement(gp, n, shape, G):
    c = cases.make_case(n, shape, False, S=2, seed=201 + n + G)
    L = 4
    A = ot.levels(c, L)
    given, W = _weights_for(c, G)
    exp = ot.expected_outcome_curve(c, A, W)
    g = cases.gpslc_object(gp, c)
    m, cov = gp.effectCurve(g, A, weights=given, outcome=True)
    mp, vp, _ = gp.predict(g, A, weights=given, outcome=True)
    if G == 1:
        assert m.shape == (2, L) and cov.shape == (2, L, L) and mp.shape == (2, L)
        m, cov, mp, vp = m[:, :, None], cov[:, :, :, None], mp[:, :, None], vp[:, :, None]
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1, 3)))               # exactly symmetric
    for l in range(L):
        assert np.array_equal(cov[:, l, l, :], vp[:, l, :])                    # the diagonal is varW to the bits
    assert np.array_equal(m, mp)
    vsc = c["yScale"]
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
    # curveSamples accepts the blocks as they are: against the pivoted-Cholesky reference on the same blocks.  The two sides run
    # the same algorithm in fp64 on the same input, so they differ by eps * cond(block): cases.draw_bounds' max(1e-9, 1e-15 cond)
    spp = 3
    z = np.random.default_rng(5).standard_normal((L, spp, 2, W.shape[0]))
    dr = gp.curveSamples(m, cov, spp, z=z)
    ref = cu.curve_samples(m, cov, spp, z)
    cond = max(np.linalg.cond(cov[s, :, :, k]) for s in range(2) for k in range(W.shape[0]) if np.any(W[k]))
    print(f"largest block condition number {cond:.3e}")
    assert np.all(np.isfinite(dr)) and np.max(np.abs(dr - ref)) <= max(1e-9, 1e-15 * cond) * np.max(np.abs(ref))


def test_other_outputs_do_not_depend_on_the_joint_covariance(gp):
    """meanW, varW, MeanITE and the draws are bit-identical with and without covW; the plain form's MeanITE and draws are the
    weighted form's."""
    c = cases.make_case(200, "UX", False, S=3, seed=231)
    A = ot.levels(c, 4)
    W = wr.weight_set(c)
    g = cases.gpslc_object(gp, c)
    kw = dict(weights=W, want_mean_ite=True, spp=4, seed=9, want_draws=True, outcome=True)
    (mw, vw, cw, mi, dr), _ = gp.api._predict_curve(g, A, **kw)
    (mw2, vw2, none, mi2, dr2), _ = gp.api._predict_curve(g, A, want_cov=False, **kw)
    assert none is None and cw is not None
    for a, b in zip((mw, vw, mi, dr), (mw2, vw2, mi2, dr2)):
        assert np.array_equal(a, b)
    ref = gp.predict(g, A, **kw)
    for a, b in zip((mw, vw, mi, dr), ref):
        assert np.array_equal(a, b)
    plain = gp.predict(g, A, want_mean_ite=True, spp=4, seed=9, want_draws=True, outcome=True)
    assert np.array_equal(plain[2], mi) and np.array_equal(plain[3], dr)
    # w = 1/n through the weighted form is the plain form's average up to the order of summation
    assert np.allclose(mw[:, :, 0], plain[0], rtol=1e-9, atol=1e-13)
    assert np.allclose(vw[:, :, 0], plain[1], rtol=1e-9, atol=1e-12 * np.max(c["yScale"]))
    # effectCurve without weights is w = 1/n
    m0, c0 = gp.effectCurve(g, A, outcome=True)
    assert np.array_equal(m0, mw[:, :, 0]) and np.array_equal(c0, cw[:, :, :, 0])


# ---- 4. ITEDistributions --------------------------------------------------------------------------------------------
def _check_dists(c, M, CV, Mr, CVr):
    yS = c["yScale"]
    for s in range(c["S"]):
        em, ec = np.max(np.abs(M[s] - Mr[s])), np.max(np.abs(CV[s] - CVr[s]))
        print(f"s={s} MeanITEs {em:.3e} of {np.max(np.abs(Mr[s])):.3e}  CovITEs {ec:.3e} (yScale {yS[s]:.3g})")
        assert em <= 1e-9 * np.max(np.abs(Mr[s])) + 1e-13
        assert ec <= 1e-9 * yS[s]
        assert np.array_equal(CV[s], CV[s].T)


@pytest.mark.parametrize("n,shape", [(129, "UX"), (129, "T"), (200, "UX"), (200, "X")])
def test_ite_distributions_outcome_against_restatement(gp, n, shape):
    c = cases.make_case(n, shape, False, S=2, seed=51 + n)
    a = 0.6
    M, CV = gp.ITEDistributions(cases.gpslc_object(gp, c), a, outcome=True)
    Mr, CVr = ot.ite_distributions_outcome(cases.samples_of(c), c["X"], c["T"], c["Y"], a)
    _check_dists(c, M, CV, Mr, CVr)


# ---- 5. GPU against GPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(129, "UX"), (200, "T")])
def test_outcome_ties_to_the_likelihood_blocks_the_contrast_and_the_ordinary_level(gp, n, shape):
    c = cases.make_case(n, shape, False, S=2, seed=55 + n)
    g = cases.gpslc_object(gp, c)
    a, b = 0.6, -0.9
    yS = c["yScale"]
    # CovOutcome - pred_noise I is CovC22 of likelihoodDistribution
    M, CV = gp.ITEDistributions(g, a, outcome=True)
    for s, p in enumerate(cases.samples_of(c)):
        C22 = gp.likelihoodDistribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], a)[7]
        e = np.max(np.abs((CV[s] - PN * np.eye(n)) - C22))
        print(f"s={s} CovOutcome - CovC22 {e:.3e} (yScale {yS[s]:.3g})")
        assert e <= 1e-9 * yS[s]
    # outcome(a) - outcome(b) is the contrast a against b
    _, _, mo = gp.predict(g, [a, b], want_mean_ite=True, outcome=True)
    _, _, mc = gp.predict(g, [a], want_mean_ite=True, baseline=b)
    for s in range(2):
        ref = mc[:, s, 0]
        e = np.max(np.abs((mo[:, s, 0] - mo[:, s, 1]) - ref))
        print(f"s={s} outcome difference - contrast {e:.3e} of {np.max(np.abs(ref)):.3e}")
        assert e <= 1e-9 * np.max(np.abs(ref)) + 1e-13
    # outcome(a) - ordinary(a) = K alpha for every level
    _, _, mr = gp.predict(g, [a, b], want_mean_ite=True)
    for s in range(2):
        k0, k1 = mo[:, s, 0] - mr[:, s, 0], mo[:, s, 1] - mr[:, s, 1]
        e = np.max(np.abs(k0 - k1))
        print(f"s={s} fitted surface from two levels {e:.3e} of {np.max(np.abs(k0)):.3e}")
        assert e <= 1e-9 * np.max(np.abs(k0)) + 1e-13


# ---- 6. draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [PN, 1e-3])
@pytest.mark.parametrize("n,shape,seed,L", ot.DRAW_CASES)
def test_draws_with_caller_normals_against_restatement(gp, n, L, shape, seed, pn):
    c = cases.make_case(n, shape, False, S=2, seed=seed)
    A = ot.levels(c, L)
    exp = ot.expected_outcome(c, A, pred_noise=pn)
    spp = 3
    z = np.random.default_rng(62).standard_normal((n, spp, c["S"], L))
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn))
    _, _, mi, dr = gp.predict(g, A, want_mean_ite=True, spp=spp, z=z, want_draws=True, outcome=True)
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
    A = ot.levels(c, 3)
    g = cases.gpslc_object(gp, c)
    kw = dict(want_mean_ite=True, spp=5, want_draws=True, outcome=True)
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
    # sampleITE / sampleSATE / predictCounterfactualEffects take the keyword
    ite = gp.sampleITE(g, A[0], samplesPerPosterior=5, seed=9, outcome=True)
    assert np.array_equal(ite, np.asfortranarray(gp.predict(g, [A[0]], seed=9, **kw)[3][0]))
    zs = np.random.default_rng(82).standard_normal(c["S"] * 4)
    got = gp.sampleSATE(g, A[0], samplesPerPosterior=4, z=zs, outcome=True)
    assert np.allclose(got, orc.sate_samples(first[0][:, 0], first[1][:, 0], 4, zs), rtol=1e-12, atol=0.0)
    dr, rng = gp.predictCounterfactualEffects(g, 2, fidelity=4, seed=9, outcome=True)
    ref = gp.predict(g, rng, spp=2, seed=9, want_draws=True, outcome=True)[3]
    assert dr.shape == (5, 200, 12) and np.array_equal(dr, ref)


# ---- 7. vector levels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("L", [1, 4, 5, 9])
def test_predict_outcome_vec_against_restatement(gp, n, L):
    """The level-block ladder 1 / 4 / 8 of the pair passes and a partial last block (L = 5, 9), on one to four tiles per side."""
    c = cases.make_case(n, "UX", False, S=2, seed=31 + L + n)
    D = vr.policy(c, L, seed=L)
    exp = ot.expected_outcome_vec(c, D, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True, outcome=True)
    _check_vec(exp, ms, vs, mi, c)


@pytest.mark.parametrize("n,shape,bt", [(129, "T", False), (200, "T", False), (129, "UX", True), (200, "UX", False)])
def test_predict_outcome_vec_policies_and_mixed_levels(gp, n, shape, bt):
    """A policy that leaves a random half as observed (d_i == T_i: the ordinary form's exact-zero rule must NOT apply), the
    observed treatment itself (the fitted surface) and two more policies; without features, and with a binary treatment."""
    c = cases.make_case(n, shape, bt, S=2, seed=36 + n)
    d, same = vr.mixed(c, seed=3)
    D = np.vstack([d[None, :], c["T"][None, :], vr.policy(c, 2, seed=2)])
    exp = ot.expected_outcome_vec(c, D, want_cov=False)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True, outcome=True)
    _check_vec(exp, ms, vs, mi, c)
    assert np.all(mi[same, :, 0] != 0.0)
    # d_i == T_i: individual i's outcome under the mixed policy is its fitted value, bit for bit (the same pairs in the same order)
    assert np.array_equal(mi[same, :, 0], mi[same, :, 1])


def test_outcome_vec_is_chunking_independent_bit_for_bit(gp):
    c = cases.make_case(200, "UX", False, S=6, seed=71)
    D = vr.policy(c, 5, seed=7)
    kw = dict(want_mean_ite=True, spp=3, seed=9, want_draws=True, outcome=True)
    first = gp.predict(cases.gpslc_object(gp, c), D, **kw)
    g4 = cases.gpslc_object(gp, c)
    g4.ctx().set_tuning(max_batch=4)
    chunked = gp.predict(g4, D, **kw)
    for a, b in zip(first, chunked):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n,shape,bt", [(129, "UX", False), (200, "T", True), (24, "X", False)])
def test_filled_vector_agrees_with_the_scalar_outcome(gp, n, shape, bt):
    c = cases.make_case(n, shape, bt, S=3, seed=51)
    g = cases.gpslc_object(gp, c)
    xs = c["doTs"]
    D = np.stack([np.full(n, x) for x in xs])
    a = gp.predict(g, xs, want_mean_ite=True, outcome=True)
    b = gp.predict(g, D, want_mean_ite=True, outcome=True)
    _check(dict(meanSATE=a[0], varSATE=a[1], meanITE=a[2]), b[0], b[1], b[2], c)


def test_ordinary_vector_effect_is_the_difference_of_two_outcomes(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=57)
    g = cases.gpslc_object(gp, c)
    d, same = vr.mixed(c, seed=5)
    _, _, mr = gp.predict(g, d[None, :], want_mean_ite=True)
    _, _, mo = gp.predict(g, np.stack([d, c["T"]]), want_mean_ite=True, outcome=True)
    diff = mo[:, :, 0] - mo[:, :, 1]
    assert np.all(diff[same] == 0.0) and np.all(mr[same, :, 0] == 0.0)
    for s in range(2):
        ref = mr[:, s, 0]
        e = np.max(np.abs(diff[:, s] - ref))
        print(f"s={s} outcome_vec(d) - outcome_vec(T) against the ordinary vector MeanITE: {e:.3e} of {np.max(np.abs(ref)):.3e}")
        assert e <= 1e-9 * np.max(np.abs(ref)) + 1e-13


def test_ite_distributions_outcome_vec_against_restatement(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=58)
    d = vr.mixed(c, seed=6)[0]
    M, CV = gp.ITEDistributions(cases.gpslc_object(gp, c), d, outcome=True)
    Mr, CVr = ot.ite_distributions_outcome(cases.samples_of(c), c["X"], c["T"], c["Y"], d)
    _check_dists(c, M, CV, Mr, CVr)


def test_outcome_vec_draws_with_caller_normals_against_restatement(gp):
    n, L = 129, 2
    c = cases.make_case(n, "UX", False, S=2, seed=61)
    D = vr.policy(c, L, seed=6)
    exp = ot.expected_outcome_vec(c, D)
    spp = 3
    z = np.random.default_rng(62).standard_normal((n, spp, c["S"], L))
    _, _, mi, dr = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True, spp=spp, z=z, want_draws=True, outcome=True)
    for s in range(c["S"]):
        for l in range(L):
            Cm = exp["covITE"][s, l]
            ref = exp["meanITE"][:, s, l][:, None] + np.linalg.cholesky(Cm) @ z[:, :, s, l]
            ev = np.linalg.eigvalsh(Cm)
            bound, _, _ = cases.draw_bounds(ev[0], ev[-1], np.linalg.norm(z[:, :, s, l]), np.linalg.norm(ref))
            assert np.linalg.norm(dr[l, :, spp * s:spp * s + spp] - ref) <= bound, (s, l)


def test_predict_outcome_vec_persistent_task_launch(gp):
    c = cases.make_case(520, "UX", False, S=5, seed=41)
    D = vr.policy(c, 3, seed=4)
    out = _forced_schedules(gp, c, lambda g: gp.predict(g, D, want_mean_ite=True, outcome=True))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    chk = [0, 4]
    exp = ot.expected_outcome_vec(c, D, samples=chk, want_cov=False)
    _check_vec(exp, *out[0], c, samples=chk)


# ---- 8. error paths -------------------------------------------------------------------------------------------------
def test_fp32_context_refuses_outcomes(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=91)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    d = c["T"] + 0.5
    with pytest.raises(gp.GPSLCError) as ei:
        gp.SATEDistributions(g, 0.6, outcome=True)
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    for call in (lambda: gp.ITEDistributions(g, 0.6, outcome=True), lambda: gp.effectCurve(g, [0.6, 0.1], outcome=True),
                 lambda: gp.SATEDistributions(g, d, outcome=True), lambda: gp.ITEDistributions(g, d, outcome=True)):
        with pytest.raises(gp.GPSLCError) as ei:
            call()
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
    last = lambda: lib.gpslc_last_error(ctx.h).decode()      # noqa: E731
    U, uy, xy, ty, ysc, yn = g._params()

    def call(doT=ok, G=0, W=None, spp=0, ms_=ms, vs_=vs, cov=None, dr=None, L=2, S_=S, prm=None):
        return lib.gpslc_predict_outcome(ctx.h, S_, *(prm or g._params()), L, _p(doT), G, _p(W), PN, spp, 0, None, _p(ms_),
                                         _p(vs_), _p(cov), None, _p(dr))

    # the scalar entry point, argument by argument
    assert call(S_=-1) == -2 and "argument #2" in last()
    assert call(prm=(None, uy, xy, ty, ysc, yn)) == -3 and "argument #3" in last()
    assert call(prm=(U, uy, None, ty, ysc, yn)) == -5 and "argument #5" in last()
    assert call(prm=(U, uy, xy, None, ysc, yn)) == -6 and "argument #6" in last()
    assert call(L=0) == -9 and "argument #9" in last()
    for bad in (np.array([0.6, np.nan]), np.array([np.inf, 0.1]), None):
        assert call(doT=bad) == -10
        assert "argument #10" in last()
    assert call(G=-1) == -11 and "argument #11" in last()
    assert call(G=0, W=w) == -11
    assert call(G=1, W=None) == -12 and "argument #12" in last()
    wbad = w.copy()
    wbad[3] = np.nan
    assert call(G=1, W=wbad) == -12
    dr = np.empty((2, n, S))
    assert call(dr=dr) == -14 and "argument #14" in last()             # ite_draws with spp < 1
    assert call(G=1, W=w, dr=dr) == -14
    assert call(cov=cw) == -19 and "argument #19" in last()            # covW without weights
    # the vector entry point
    D = np.asfortranarray(np.stack([c["T"] + 0.5, c["T"]]).T)
    Dbad = D.copy()
    Dbad[5, 1] = np.nan

    def callv(doT=D, L=2, spp=0, dr=None, S_=S, prm=None):
        return lib.gpslc_predict_outcome_vec(ctx.h, S_, *(prm or g._params()), L, _p(doT), PN, spp, 0, None, _p(ms), _p(vs),
                                             None, _p(dr))

    assert callv(S_=-1) == -2
    assert callv(prm=(None, uy, xy, ty, ysc, yn)) == -3
    assert callv(prm=(U, uy, None, ty, ysc, yn)) == -5
    assert callv(prm=(U, uy, xy, None, ysc, yn)) == -6
    assert callv(L=0) == -9
    for bad in (None, Dbad):
        assert callv(doT=bad) == -10 and "argument #10" in last()
    assert callv(dr=dr) == -12 and "argument #12" in last()
    # the two ITE-distribution entry points
    M = np.empty((S, n))
    for bad in (float("nan"), float("inf")):
        assert lib.gpslc_ite_distributions_outcome(ctx.h, S, *g._params(), bad, PN, _p(M), None) == -9
        assert "argument #9" in last()
    assert lib.gpslc_ite_distributions_outcome(ctx.h, -1, *g._params(), 0.6, PN, _p(M), None) == -2
    assert lib.gpslc_ite_distributions_outcome(ctx.h, S, U, uy, xy, None, ysc, yn, 0.6, PN, _p(M), None) == -6
    dv = np.ascontiguousarray(D[:, 0])
    dvbad = dv.copy()
    dvbad[2] = np.inf
    for bad in (None, dvbad):
        assert lib.gpslc_ite_distributions_outcome_vec(ctx.h, S, *g._params(), _p(bad), PN, _p(M), None) == -9
        assert "argument #9" in last()
    assert lib.gpslc_ite_distributions_outcome_vec(ctx.h, -1, *g._params(), _p(dv), PN, _p(M), None) == -2
    # the good calls: plain, weighted with the covariance, vector, and the two distributions
    assert call() == 0
    mw, vw = np.empty((S, 2, 1), order="F"), np.empty((S, 2, 1), order="F")
    assert call(G=1, W=w, ms_=mw, vs_=vw, cov=cw) == 0
    assert np.allclose(mw[:, :, 0], ms, rtol=1e-9, atol=1e-13) and np.array_equal(cw[:, 0, 0, 0], vw[:, 0, 0])
    assert callv() == 0 and np.all(np.isfinite(ms)) and np.all(vs > 0)
    assert lib.gpslc_ite_distributions_outcome(ctx.h, S, *g._params(), 0.6, PN, _p(M), None) == 0 and np.all(np.isfinite(M))
    assert lib.gpslc_ite_distributions_outcome_vec(ctx.h, S, *g._params(), _p(dv), PN, _p(M), None) == 0 and np.all(np.isfinite(M))
