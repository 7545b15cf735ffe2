"""Per-individual interventions (gpslc_predict_vec, gpslc_ite_distributions_vec, gpslc_likelihood_distribution_vec and the
Python mirror's vector routing) against the dense restatement in tests/vector_restatement.py."""
import ctypes as C

import numpy as np
import pytest

import cases
import gpslc_oracle as orc
import vector_restatement as vr

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


def _check(exp, ms, vs, mi, case, samples=None, tight=1e-9):
    """The bounds test_gpu_estimation._check_against applies to the scalar path."""
    yS = case["yScale"]
    L = ms.shape[1]
    for s in (range(case["S"]) if samples is None else samples):
        for l in range(L):
            rm, rv = exp["meanSATE"][s, l], exp["varSATE"][s, l]
            assert abs(ms[s, l] - rm) <= 1e-6 * abs(rm) + 1e-12, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= 1e-6 * abs(rv) + 1e-9 * yS[s], (s, l, vs[s, l], rv)
            assert abs(ms[s, l] - rm) <= tight * abs(rm) + 1e-13, (s, l, ms[s, l], rm)
            assert abs(vs[s, l] - rv) <= tight * abs(rv) + 1e-12 * yS[s], (s, l, vs[s, l], rv)
            if mi is not None:
                ref = exp["meanITE"][:, s, l]
                assert np.max(np.abs(mi[:, s, l] - ref)) <= 1e-6 * np.max(np.abs(ref)) + 1e-12, (s, l)
                assert np.max(np.abs(mi[:, s, l] - ref)) <= tight * np.max(np.abs(ref)) + 1e-13, (s, l)


# ---- 1. dense blocks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [1, 24, 129, 200])
def test_likelihood_distribution_blocks_vec(gp, n, shape, bt):
    c = cases.make_case(n, shape, bt, S=1, seed=11 + n)
    p = cases.samples_of(c)[0]
    d = vr.policy(c, 2, seed=n)[1]
    if bt:
        d = d.astype(bool)                     # a Vector{Bool}: 0 / 1
    ref = vr.likelihood_distribution_vec(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], d)
    got = gp.likelihoodDistribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], d)
    for name, a, b in zip(("Y", "CovWW", "CovWWs", "CovWWp", "C11", "C12", "C21", "C22"), got, ref):
        assert np.max(np.abs(a - b)) <= 1e-9 * p.yScale, (name, np.max(np.abs(a - b)))


# ---- 2. exact zeros -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
def test_exact_zeros_when_the_intervention_is_the_observed_treatment(gp, shape, bt):
    n = 150
    c = cases.make_case(n, shape, bt, S=2, seed=21)
    p = cases.samples_of(c)[0]
    T = c["T"]
    m, Cv = gp.conditionalITE(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], T, c["Y"], T.copy())
    assert np.array_equal(m, np.zeros(n)) and np.array_equal(Cv, np.zeros((n, n)))
    g = cases.gpslc_object(gp, c)
    M, CV = gp.ITEDistributions(g, T.copy())
    assert np.all(M == 0.0)
    for s in range(c["S"]):
        assert np.array_equal(CV[s], PN * np.eye(n))
    ms, vs = gp.SATEDistributions(g, T.copy())
    assert np.all(ms == 0.0)
    assert np.all(vs == (n * PN) / (n * n))
    # a mixed policy: MeanITE_i is exactly 0.0 wherever d_i == T_i, on every path that yields it
    d, same = vr.mixed(c, seed=3)
    M, _ = gp.ITEDistributions(g, d)
    assert np.all(M[:, same] == 0.0) and np.any(M[:, ~same] != 0.0)
    _, _, mi = gp.predict(g, np.stack([d, T]), want_mean_ite=True)
    assert np.all(mi[same, :, 0] == 0.0) and np.all(mi[:, :, 1] == 0.0)


# ---- 3. predict against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(129, 1), (129, 5), (129, 40), (400, 1), (400, 5), (400, 40), (24, 130)])
@pytest.mark.parametrize("bt", [False, True])
def test_predict_vec_against_restatement(gp, n, L, bt):
    c = cases.make_case(n, "UX", bt, S=3, seed=31 + L)
    D = vr.policy(c, L, seed=L)
    exp = vr.expected_vec(c, D)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True)
    _check(exp, ms, vs, mi, c)


def test_predict_vec_persistent_task_launch(gp):
    """S >= 256 at five tiles per side: the default schedule factorises the chunk in one persistent launch."""
    c = cases.make_case(520, "UX", False, S=256, seed=41)
    D = vr.policy(c, 3, seed=4)
    chk = [0, 129, 255]
    exp = vr.expected_vec(c, D, samples=chk)
    ms, vs, mi = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True)
    _check(exp, ms, vs, mi, c, samples=chk)


# ---- 4. scalar equivalence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,bt", [(129, "UX", False), (200, "T", True), (24, "X", False)])
def test_filled_vector_agrees_with_the_scalar_level(gp, n, shape, bt):
    c = cases.make_case(n, shape, bt, S=3, seed=51)
    g = cases.gpslc_object(gp, c)
    xs = c["doTs"]
    D = np.stack([np.full(n, x) for x in xs])
    a = gp.predict(g, xs, want_mean_ite=True, spp=4, seed=7, want_draws=True)
    b = gp.predict(g, D, want_mean_ite=True, spp=4, seed=7, want_draws=True)
    ref = dict(meanSATE=a[0], varSATE=a[1], meanITE=a[2])
    _check(ref, b[0], b[1], b[2], c)
    exp = cases.oracle_expected(c)
    for s in range(c["S"]):
        for l in range(len(xs)):
            ev = np.linalg.eigvalsh(exp["covITE"][s, l])
            cols = slice(4 * s, 4 * s + 4)
            bound, _, _ = cases.draw_bounds(ev[0], ev[-1], 2 * np.sqrt(4 * n), np.linalg.norm(a[3][l, :, cols]))
            assert np.linalg.norm(b[3][l, :, cols] - a[3][l, :, cols]) <= bound, (s, l)


# ---- 5. draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(129, 1), (200, 3)])
def test_draws_with_caller_normals_against_restatement(gp, n, L):
    c = cases.make_case(n, "UX", False, S=2, seed=61)
    D = vr.policy(c, L, seed=6)
    exp = vr.expected_vec(c, D)
    spp = 3
    z = np.random.default_rng(62).standard_normal((n, spp, c["S"], L))
    _, _, mi, dr = gp.predict(cases.gpslc_object(gp, c), D, want_mean_ite=True, spp=spp, z=z, want_draws=True)
    for s in range(c["S"]):
        for l in range(L):
            Cm = exp["covITE"][s, l]
            Lc = np.linalg.cholesky(Cm)
            ref = exp["meanITE"][:, s, l][:, None] + Lc @ z[:, :, s, l]
            ev = np.linalg.eigvalsh(Cm)
            bound, _, _ = cases.draw_bounds(ev[0], ev[-1], np.linalg.norm(z[:, :, s, l]), np.linalg.norm(ref))
            assert np.linalg.norm(dr[l, :, spp * s:spp * s + spp] - ref) <= bound, (s, l)


def test_seeded_draws_are_reproducible_and_chunking_independent(gp):
    c = cases.make_case(200, "UX", False, S=6, seed=71)
    D = vr.policy(c, 3, seed=7)
    g = cases.gpslc_object(gp, c)
    xs = np.array([0.2, 0.6])
    first = gp.predict(g, D, want_mean_ite=True, spp=5, seed=9, want_draws=True)
    again = gp.predict(g, D, want_mean_ite=True, spp=5, seed=9, want_draws=True)
    scal = gp.predict(g, xs, want_mean_ite=True, spp=5, seed=9, want_draws=True)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    g4 = cases.gpslc_object(gp, c)
    g4.ctx().set_tuning(max_batch=4)
    chunked = gp.predict(g4, D, want_mean_ite=True, spp=5, seed=9, want_draws=True)
    scal_chunked = gp.predict(g4, xs, want_mean_ite=True, spp=5, seed=9, want_draws=True)
    if all(np.array_equal(a, b) for a, b in zip(scal, scal_chunked)):      # the scalar path is bit-identical across chunkings
        for a, b in zip(first, chunked):
            assert np.array_equal(a, b)


# ---- 6. public surface ----------------------------------------------------------------------------------------------
def test_sample_sate_and_ite_take_the_vector(gp):
    """This used to return the answer for the scalar doT[0]."""
    n = 129
    c = cases.make_case(n, "UX", False, S=3, seed=81)
    g = cases.gpslc_object(gp, c)
    d = c["T"] + 0.5
    d[: n // 2] = c["T"][: n // 2]
    exp = vr.expected_vec(c, d[None, :])
    z = np.random.default_rng(82).standard_normal(c["S"] * 4)
    got = gp.sampleSATE(g, d, samplesPerPosterior=4, z=z)
    ref = orc.sate_samples(exp["meanSATE"][:, 0], exp["varSATE"][:, 0], 4, z)
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-12)
    wrong = gp.sampleSATE(g, d[0], samplesPerPosterior=4, z=z)
    assert not np.allclose(got, wrong, rtol=1e-3)
    zi = np.random.default_rng(83).standard_normal((n, c["S"] * 4))
    ite = gp.sampleITE(g, d, samplesPerPosterior=4, z=zi)
    M, CV = vr.ite_distributions_vec(cases.samples_of(c), c["X"], c["T"], c["Y"], d)
    ref = orc.ite_samples(M, CV, 4, zi)
    assert np.max(np.abs(ite - ref)) <= 1e-6 * np.max(np.abs(ref))
    with pytest.raises(ValueError, match=f"n = {n}"):
        gp.sampleSATE(g, d[:-1])
    with pytest.raises(NotImplementedError):
        gp.predict(g, d[None, :], devices=[0, 0])


def test_fp32_context_refuses_vector_levels(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=91)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.SATEDistributions(g, c["T"] + 0.5)
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    with pytest.raises(gp.GPSLCError):
        gp.ITEDistributions(g, c["T"] + 0.5)
    gp.SATEDistributions(g, 0.5)               # the scalar path of the same context keeps working


def test_c_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=92)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    lib = ctx.lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, S = 24, 2
    ms, vs = np.empty(S), np.empty(S)
    bad = np.tile(c["T"], 1).copy()
    bad[5] = np.nan
    for doT in (None, bad):
        assert lib.gpslc_predict_vec(ctx.h, S, *g._params(), 1, p(doT), PN, 0, 0, None, p(ms), p(vs), None, None) == -10
        assert "argument #10" in lib.gpslc_last_error(ctx.h).decode()
        M = np.empty((S, n))
        assert lib.gpslc_ite_distributions_vec(ctx.h, S, *g._params(), p(doT), PN, p(M), None) == -9
        blk = np.empty((n, n))
        pr = cases.samples_of(c)[0]
        U = np.asfortranarray(pr.U)
        uy, xy = np.ascontiguousarray(pr.uyLS), np.ascontiguousarray(pr.xyLS)
        assert lib.gpslc_likelihood_distribution_vec(ctx.h, p(U), p(uy), p(xy), pr.tyLS, pr.yScale, pr.yNoise, p(doT),
                                                     p(blk), None, None, None, None, None, None) == -8
    assert lib.gpslc_predict_vec(ctx.h, S, *g._params(), 0, p(c["T"]), PN, 0, 0, None, p(ms), p(vs), None, None) == -9
