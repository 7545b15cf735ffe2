"""The HIP path on inputs off the unit scale.  Every other seeded case draws its covariates standard-normal, its lengthscales
in [0.25, 10] and Y, yScale, yNoise of order one: the kernels are exercised widely in shape and at one point in value.  The RBF
model sees differences over lengthscales only, so (tests/offscale.py has the transforms)
  a. a change of a column's unit (powers of two on the column and its lengthscale) must not move a bit of any fp64 output;
  b. a change of the outcome's unit (Y by 2**k, yScale / yNoise / jitter by 4**k) scales every fp64 output by an exact power
     of two, under the per-column schedule and the persistent launch — yLogpdf (a log) against the oracle instead;
  c. data shifted by up to +-1000 per column answers like the oracle of the shifted data (SURVEY §8d tolerances and 1e-9, as
     tests/test_gpu_estimation.py) and like the GPU's own unshifted answer to 1e-9;
  d. the mixed-precision mode (GPSLC_FLAG_FP32_KERNEL) keeps its 1e-6 budget wherever the origin is: features are centred per
     column in fp64 before the fp32 rounding, so a shift that is exact in fp64 does not move a bit of its outputs;
  e. the two exponential routines of gp_math.h over their whole domain: reduction breakpoints, the -800 clamp, subnormal and zero
     results.
tests/test_offscale_reference.py pins the oracle's side of every tolerance here on the CPU.
The work replaced: src/kernel.jl:13-59, src/likelihood.jl:8-174, src/estimation.jl:36-163, src/model_likelihood.jl:83-120."""
import numpy as np
import pytest

import cases
import gpslc_oracle as orc
import offscale
from offscale import bits_equal, bits_differ

pytestmark = pytest.mark.gpu

E_X, E_U, E_T = (20, -20, 7), (-3, 11), 9
LD_BLOCKS = ("CovWW", "CovWWs", "CovWWp", "CovC11", "CovC12", "CovC21", "CovC22")


def _same(name, a, b):
    assert bits_equal(a, b), f"{name}: {bits_differ(a, b)}"


def _enrich(c, L9):
    """The case with a sweep of nine levels (continuous T), a baseline per level and a (2, n) level array beside its two levels."""
    n = c["n"]
    rng = np.random.Generator(np.random.Philox(77 + n))
    if c["binary_t"]:
        lv = (rng.random((2, n)) < 0.5).astype(np.float64)
        return dict(c, baseline=np.array([1.0, 0.0]), levels=lv)
    return dict(c, baseline=np.array([0.9, -0.2]), levels=rng.uniform(-1.0, 1.0, (2, n)), sweep=L9)


def _all_prediction_outputs(gp, c):
    """name -> array for every prediction entry point on one object of the case."""
    g = cases.gpslc_object(gp, c)
    n = c["n"]
    W = np.stack([np.full(n, 1.0 / n), (np.arange(n) % 3 == 0) / float(len(range(0, n, 3)))])
    out = {}

    def put(prefix, names, arrays):
        for k, a in zip(names, arrays):
            out[f"{prefix}.{k}"] = a
    four = ("meanSATE", "varSATE", "MeanITE", "draws")
    put("L2", four, gp.predict(g, c["doTs"], want_mean_ite=True, spp=3, seed=5, want_draws=True))
    if c.get("sweep") is not None:
        put("L9", four, gp.predict(g, c["sweep"], want_mean_ite=True, spp=3, seed=6, want_draws=True))
    put("curve", ("mean", "cov"), gp.effectCurve(g, c["sweep"] if c.get("sweep") is not None else c["doTs"]))
    put("baseline", four, gp.predict(g, c["doTs"], baseline=c["baseline"], want_mean_ite=True, spp=3, seed=7, want_draws=True))
    put("weights", four[:3], gp.predict(g, c["doTs"], weights=W, want_mean_ite=True))
    put("levels", four, gp.predict(g, c["levels"], want_mean_ite=True, spp=3, seed=8, want_draws=True))
    put("itedist", ("MeanITEs", "CovITEs"), gp.ITEDistributions(g, float(c["doTs"][1])))
    g.ctx().close()
    return out


def _likelihood_blocks(gp, c, s=1):
    p = cases.samples_of(c)[s]
    return dict(zip(LD_BLOCKS, gp.likelihoodDistribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"],
                                                         float(c["doTs"][1]))[1:]))


# ---------------------------------------------------------------------------------------------------------------------------
# a. a change of units is invisible, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
UNIT_CASES = [(129, "UX", False), (200, "U", False), (200, "X", False), (129, "T", False), (200, "UX", True), (129, "X", True)]


@pytest.mark.parametrize("n,shape,bt", UNIT_CASES)
def test_a_change_of_units_moves_no_bit(gp, n, shape, bt):
    """x * (1 / ls), (d * d) * wt and 1 / (tl * tl) keep every bit under powers of two on a column and its lengthscale (a binary T
    keeps its unit), so every fp64 output of every prediction entry point and all seven likelihood blocks must too."""
    c = _enrich(cases.make_case(n, shape, bt, S=3, seed=810 + n + bt), np.linspace(-0.7, 0.9, 9))
    r = offscale.rescale_features(c, E_X, E_U, 0 if bt else E_T)
    plain, scaled = _all_prediction_outputs(gp, c), _all_prediction_outputs(gp, r)
    assert sorted(plain) == sorted(scaled) and len(plain) == (19 if bt else 23)
    for k in plain:
        assert np.all(np.isfinite(plain[k])), k
        _same(k, scaled[k], plain[k])
    lp, ls = _likelihood_blocks(gp, c), _likelihood_blocks(gp, r)
    for k in LD_BLOCKS:
        _same(k, ls[k], lp[k])


@pytest.mark.parametrize("n", [150, 700])          # the single-workgroup kernel, the tiled path
@pytest.mark.parametrize("shape", ["UX", "U", "X", "T"])
def test_a_change_of_units_moves_no_bit_of_the_node_score(gp, n, shape):
    c = cases.make_case(n, shape, False, S=3, seed=820 + n)
    r = offscale.rescale_features(c, E_X, E_U, E_T)
    _same("logpdf", gp.yLogpdf(cases.gpslc_object(gp, r)), gp.yLogpdf(cases.gpslc_object(gp, c)))


# ---------------------------------------------------------------------------------------------------------------------------
# b. a change of the outcome's unit scales the answer exactly
# ---------------------------------------------------------------------------------------------------------------------------
def _outcome_outputs(gp, c, pcn, tiles, with_cov):
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pcn))
    g.ctx().set_task_schedule(2, tiles, 1, 0)
    out = dict(zip(("meanSATE", "varSATE", "MeanITE", "draws"),
                   gp.predict(g, c["doTs"], want_mean_ite=True, spp=2, seed=9, want_draws=True)))
    if with_cov:
        out["MeanITEs"], out["CovITEs"] = gp.ITEDistributions(g, float(c["doTs"][0]))
        out["curve_mean"], out["curve_cov"] = gp.effectCurve(g, np.linspace(-0.7, 0.9, 5))
        out["logpdf"] = gp.yLogpdf(g)
    g.ctx().close()
    return out


SECOND_ORDER = ("varSATE", "CovITEs", "curve_cov")      # scale with 4**k; every other output with 2**k


@pytest.mark.parametrize("k", [-9, 11])
@pytest.mark.parametrize("schedule", ["columns", "tasks"])
def test_the_outcomes_unit_scales_every_output_by_an_exact_power_of_two(gp, schedule, k):
    """Y -> 2**k Y, yScale / yNoise / jitter -> 4**k: A -> 4**k A, and the Cholesky (sqrt / rsqrt steps on the mantissa), the
    solves and the epilogue are homogeneous in the matrix's scale, so MeanITE, meanSATE and the draws come out times 2**k and
    varSATE, CovITE and the curve's covariance times 4**k, bit for bit.  `columns`: one launch per tile column (n = 200, S = 3);
    `tasks`: the persistent launch at its default threshold (S = 256 matrices at n = 200).  yLogpdf holds a log and is not
    homogeneous: against the oracle of the rescaled case at the golden tolerance."""
    tasks = schedule == "tasks"
    c = cases.make_case(200, "UX", False, S=256 if tasks else 3, seed=830)
    r = offscale.rescale_outcome(c, k)
    pcn = 1e-3
    plain = _outcome_outputs(gp, c, pcn, 32 if tasks else 0, not tasks)
    scaled = _outcome_outputs(gp, r, pcn * 4.0 ** k, 32 if tasks else 0, not tasks)
    for name in plain:
        if name == "logpdf":
            continue
        f = 4.0 ** k if name in SECOND_ORDER else 2.0 ** k
        assert np.all(np.isfinite(plain[name])), name
        _same(name, scaled[name], plain[name] * f)
    if not tasks:
        ref = np.array([orc.y_logpdf(p.uyLS, p.xyLS, p.tyLS, p.yScale, p.yNoise, p.U, r["X"], r["T"], r["Y"])
                        for p in cases.samples_of(r)])
        assert np.allclose(scaled["logpdf"], ref, rtol=1e-10, atol=1e-9), (scaled["logpdf"], ref)


# ---------------------------------------------------------------------------------------------------------------------------
# c. shifted data against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
PCN_DRAWS = 1e-3


def _shift_outputs(gp, c, z):
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=PCN_DRAWS))
    ms, vs, mi, dr = gp.predict(g, c["doTs"], want_mean_ite=True, spp=z.shape[1], z=z, want_draws=True)
    M, Cv = gp.ITEDistributions(g, float(c["doTs"][1]))
    lp = gp.yLogpdf(g)
    g.ctx().close()
    return dict(ms=ms, vs=vs, mi=mi, dr=dr, M=M, Cv=Cv, lp=lp)


@pytest.mark.parametrize("n,shape,bt", offscale.SHIFT_CASES)
def test_shifted_data_against_the_oracle_and_the_unshifted_answer(gp, n, shape, bt):
    """X, U by up to +-1000 per column (signs and sizes differ), T and the levels by 1000 (a binary T stays): predict with the
    caller's normals at jitter 1e-3, ITEDistributions and yLogpdf against the literal restatement OF THE SHIFTED CASE — SURVEY
    §8d's tolerances and 1e-9, draws under cases.draw_bounds — and against the GPU's own answer on the plain case at 1e-9.  The
    fp64 kernels take x * (1 / ls) before the difference: eps |x| / ls = 1e-13 at 1000 lengthscales from the origin."""
    c, cs = offscale.shift_case_pair(n, shape, bt)
    S, L, spp = c["S"], len(c["doTs"]), 2
    z = np.random.default_rng(n).standard_normal((n, spp, S, L))
    exp = cases.oracle_expected(cs, PCN_DRAWS)
    got, got0 = _shift_outputs(gp, cs, z), _shift_outputs(gp, c, z)
    yS = c["yScale"]
    for o in (got, got0):                                   # both against the oracle (which test 2 of the CPU file ties together)
        for s in range(S):
            for l in range(L):
                rm, rv, ref = exp["meanSATE"][s, l], exp["varSATE"][s, l], exp["meanITE"][:, s, l]
                assert abs(o["ms"][s, l] - rm) <= 1e-6 * abs(rm) + 1e-12
                assert abs(o["vs"][s, l] - rv) <= 1e-6 * abs(rv) + 1e-9 * yS[s]
                assert abs(o["ms"][s, l] - rm) <= 1e-9 * abs(rm) + 1e-13
                assert abs(o["vs"][s, l] - rv) <= 1e-9 * abs(rv) + 1e-12 * yS[s]
                assert np.max(np.abs(o["mi"][:, s, l] - ref)) <= 1e-6 * np.max(np.abs(ref)) + 1e-12
                assert np.max(np.abs(o["mi"][:, s, l] - ref)) <= 1e-9 * np.max(np.abs(ref)) + 1e-13
                ev = np.linalg.eigvalsh(exp["covITE"][s, l])
                Lc = np.linalg.cholesky(exp["covITE"][s, l])
                for d in range(spp):
                    zz = z[:, d, s, l]
                    rd = ref + Lc @ zz
                    bound, tight, cond = cases.draw_bounds(ev[0], ev[-1], np.linalg.norm(zz), np.linalg.norm(rd))
                    err = np.linalg.norm(o["dr"][l, :, spp * s + d] - rd)
                    assert err <= bound and (tight is None or err <= tight), (s, l, d, err, bound, tight, cond)
            assert np.max(np.abs(o["M"][s] - exp["meanITE"][:, s, 1])) <= 1e-9 * np.max(np.abs(exp["meanITE"][:, s, 1])) + 1e-13
            assert np.max(np.abs(o["Cv"][s] - exp["covITE"][s, 1])) <= 1e-9 * yS[s]
            assert np.array_equal(o["Cv"][s], o["Cv"][s].T)
        assert np.allclose(o["lp"], exp["logpdf"], rtol=1e-10, atol=1e-9)
    # the GPU's own plain answer, 1e-9
    assert np.all(np.abs(got["ms"] - got0["ms"]) <= 1e-9 * np.abs(got0["ms"]) + 1e-13)
    assert np.all(np.abs(got["vs"] - got0["vs"]) <= 1e-9 * np.abs(got0["vs"]) + 1e-12 * yS[:, None])
    assert np.max(np.abs(got["mi"] - got0["mi"])) <= 1e-9 * np.max(np.abs(got0["mi"])) + 1e-13
    assert np.max(np.abs(got["dr"] - got0["dr"])) <= 1e-9 * np.max(np.abs(got0["dr"])) + 1e-13
    assert np.max(np.abs(got["M"] - got0["M"])) <= 1e-9 * np.max(np.abs(got0["M"])) + 1e-13
    assert np.all(np.max(np.abs(got["Cv"] - got0["Cv"]), axis=(1, 2)) <= 1e-9 * yS)
    assert np.allclose(got["lp"], got0["lp"], rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# d. the mixed-precision budget holds wherever the origin is
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_cases():
    """name -> (case, oracle of the plain case), computed once and left unchanged."""
    return {k: (c, cases.oracle_expected(c)) for k, c in offscale.fp32_base_cases().items()}


def fp32_drifts(gp, c, exp):
    """(rel meanSATE, rel MeanITE, varSATE within its bound) of an fp32-kernel context against the fp64 oracle, as
    test_fp32_kernel_mode_drift_and_identities measures them."""
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    ms, vs, mi = gp.predict(g, c["doTs"], want_mean_ite=True)
    g.ctx().close()
    rel_m = float(np.max(np.abs(ms - exp["meanSATE"]) / np.abs(exp["meanSATE"])))
    rel_i = float(np.max(np.abs(mi - exp["meanITE"])) / np.max(np.abs(exp["meanITE"])))
    v_ok = bool(np.all(np.abs(vs - exp["varSATE"]) <= 1e-6 * np.abs(exp["varSATE"]) + 1e-9 * c["yScale"][:, None]))
    return rel_m, rel_i, v_ok


@pytest.mark.parametrize("sh", offscale.FP32_SHIFTS)
@pytest.mark.parametrize("name", ["main_L2", "main_L17", "X14", "binary"])
def test_fp32_kernel_mode_keeps_its_budget_wherever_the_origin_is(gp, fp32_cases, name, sh):
    """The three assertions of test_fp32_kernel_mode_drift_and_identities with X, U, T and the levels moved by 0, 100 and 1e4,
    against the fp64 oracle of the plain case (the oracle does not notice the origin: test_offscale_reference.py).  main: that
    test's n = 300 case at L = 2 and at L = 17 (the 16-level VALU path); X14: shape X with nX = 14 (the float runtime-F Gram
    path); binary: a binary treatment.  Before the features were centred per column the kernels rounded x / ls to fp32 and then
    took the difference: the drift grew with |x| / ls (DESIGN.md §4 has the figures measured then and now)."""
    c, exp = fp32_cases[name]
    rel_m, rel_i, v_ok = fp32_drifts(gp, offscale.fp32_shifted(c, sh), exp)
    print(f"fp32 drift {name} shift {sh:g}: meanSATE {rel_m:.3e} MeanITE {rel_i:.3e} varSATE ok {v_ok}")
    assert 1e-12 < rel_m < 1e-6, rel_m
    assert rel_i < 1e-6, rel_i
    assert v_ok


@pytest.mark.parametrize("name", ["main_L2", "main_L17"])
def test_fp32_kernel_mode_does_not_see_an_exact_shift(gp, name):
    """Inputs on a 2**-12 grid moved by 2**13 in every column: the sums are exact in fp64, so every centred value, every
    treatment difference and with them every output of the fp32 mode is the same number — bit for bit."""
    q = offscale.quantise(offscale.fp32_base_cases()[name], 12)
    s = offscale.fp32_shifted(q, 2.0 ** 13)
    outs = []
    for c in (q, s):
        g = cases.gpslc_object(gp, c, fp32_kernel=True)
        outs.append(gp.predict(g, c["doTs"], want_mean_ite=True) + (gp.yLogpdf(g),))
        g.ctx().close()
    for k, a, b in zip(("meanSATE", "varSATE", "MeanITE", "logpdf"), outs[1], outs[0]):
        assert np.all(np.isfinite(b)), k
        _same(k, a, b)


def test_fp32_exact_zeros_far_from_the_origin(gp):
    """doT == T everywhere gives exact zeros in the fp32 mode (expf(-0) == 1) at T = doT = 1000.25 as it does at 0.25."""
    n = 130
    rng = np.random.default_rng(0)
    g = gp.GPSLCObject(rng.standard_normal((n, 2)) + 1000.0, np.full(n, 1000.25), rng.standard_normal(n),
                       rng.standard_normal((n, 1, 1)) - 1000.0, [[1.3]], [[0.9], [1.7]], [0.8], [0.6], [1.1], fp32_kernel=True)
    ms, vs, mi = gp.predict(g, [1000.25], want_mean_ite=True)
    assert np.all(ms == 0.0) and np.all(mi == 0.0)


def test_fp32_node_score_wherever_the_origin_is(gp):
    """yLogpdf at n = 150, which an fp32 context sends down the tiled path (Gram build in fp32).  The yardstick is the plain fp32
    context's own deviation from the fp64 oracle, measured here: the shifted contexts stay within 4 x the largest of the three
    samples' deviations plus 1e-9 |logpdf| — centring on the first element may double a feature's magnitude, hence quadruple the
    rounding error of its square.  Measured on an MI355X (|logpdf| = 228, 232, 250): plain deviations
    2.1e-7, 7.4e-7, 1.8e-7, and the same three figures to every digit at shifts 100 and 1e4; before the centring the shifted
    contexts deviated by up to 1.6e-5 and 5.9e-4."""
    c = cases.make_case(150, "UX", False, S=3, seed=850)
    ref = cases.oracle_expected(c)["logpdf"]
    lp = {}
    for sh in offscale.FP32_SHIFTS:
        g = cases.gpslc_object(gp, offscale.fp32_shifted(c, sh), fp32_kernel=True)
        lp[sh] = gp.yLogpdf(g)
        g.ctx().close()
    dev0 = np.abs(lp[0.0] - ref)
    print("fp32 logpdf deviations:", {sh: np.abs(v - ref) for sh, v in lp.items()}, "of", ref)
    assert 0 < dev0.max() <= 1e-6 * np.max(np.abs(ref))          # a different arithmetic, inside the mode's budget
    for sh in offscale.FP32_SHIFTS[1:]:
        assert np.all(np.abs(lp[sh] - ref) <= 4.0 * dev0.max() + 1e-9 * np.abs(ref)), (sh, np.abs(lp[sh] - ref), dev0)


# ---------------------------------------------------------------------------------------------------------------------------
# e. the exponential over its whole domain
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["T", "X"])
def test_exponential_over_its_whole_domain(gp, shape):
    """Row 0 of CovWW with yScale = 1 is the raw kernel value exp(-a_j): a_j = (t_0 - t_j)^2 / tyLS^2 through gp_rho at shape T,
    the feature sum fma(d, d, 0) of the tile-build body at shape X (one column, lengthscale 1, every T equal: e = exp(-0) = 1).
    Both evaluate gp_exp_neg.  Against exp in long double of the argument formed with the kernel's own fp64 operations: exactly 1
    at a = 0, within 1 ulp where the reference is normal (gp_math.h's bound), within one subnormal spacing where it is subnormal,
    exactly 0 beyond, and finite, non-negative and non-increasing in a throughout."""
    t = offscale.exp_ladder_t()
    n = t.shape[0]
    a, ref = offscale.exp_reference(t)
    Y = np.random.default_rng(1).standard_normal(n)
    if shape == "T":
        out = gp.likelihoodDistribution(None, None, 1.0, 1.0, 1.0, None, None, t, Y, 0.5)
    else:
        out = gp.likelihoodDistribution(None, [1.0], 1.0, 1.0, 1.0, None, t[:, None], np.full(n, 0.5), Y, 0.5)
    row = np.ascontiguousarray(out[1][0, :])
    assert bits_equal(row[:1], np.ones(1))
    assert np.all(np.isfinite(row)) and np.all(row >= 0.0) and not np.any(np.signbit(row))
    tiny = float(np.finfo(np.float64).tiny)
    normal, zero = ref >= tiny, ref == 0.0
    sub = ~normal & ~zero
    assert normal.sum() >= 30 and sub.sum() >= 50 and zero.sum() >= 8
    err = np.abs(row - ref)
    assert np.all(err[normal] <= np.spacing(ref[normal])), (a[normal][np.argmax(err[normal] / np.spacing(ref[normal]))],)
    assert np.all(err[sub] <= 2.0 ** -1074), (a[sub], row[sub], ref[sub])
    assert bits_equal(row[zero], np.zeros(int(zero.sum()))), (a[zero], row[zero])
    order = np.argsort(a, kind="stable")
    assert np.all(np.diff(row[order]) <= 0.0), a[order][1:][np.diff(row[order]) > 0.0]
    assert np.array_equal(out[1], out[1].T)


@pytest.fixture(scope="module")
def bridged():
    """name -> (case, oracle): two clusters 60 lengthscales apart with bridge points, at L = 2 and L = 9."""
    return {k: (c, cases.oracle_expected(c)) for k, c in offscale.bridged_cases().items()}


@pytest.mark.parametrize("name", ["L2", "L9"])
def test_table_driven_exponential_where_the_result_is_subnormal_or_zero(gp, bridged, name):
    """gp_exp_neg_tab has no raw output: the Gram build and the MeanITE pass (L = 2: the VALU kernel, L = 9: the MFMA form) on a
    case whose pair exponents run from 0 past -600 .. -900 (the ldexp into the subnormal range, the -800 clamp) to -3600, on an
    fp64 context at the tolerances of (c) and on an fp32 context at those of (d).  Every output finite."""
    c, exp = bridged[name]
    g = cases.gpslc_object(gp, c)
    ms, vs, mi = gp.predict(g, c["doTs"], want_mean_ite=True)
    lp = gp.yLogpdf(g)
    g.ctx().close()
    assert all(np.all(np.isfinite(v)) for v in (ms, vs, mi, lp))
    yS = c["yScale"]
    for s in range(c["S"]):
        for l in range(len(c["doTs"])):
            rm, rv, ref = exp["meanSATE"][s, l], exp["varSATE"][s, l], exp["meanITE"][:, s, l]
            assert abs(ms[s, l] - rm) <= 1e-9 * abs(rm) + 1e-13
            assert abs(vs[s, l] - rv) <= 1e-9 * abs(rv) + 1e-12 * yS[s]
            assert np.max(np.abs(mi[:, s, l] - ref)) <= 1e-9 * np.max(np.abs(ref)) + 1e-13
    assert np.allclose(lp, exp["logpdf"], rtol=1e-10, atol=1e-9)
    rel_m, rel_i, v_ok = fp32_drifts(gp, c, exp)
    print(f"fp32 drift bridged {name}: meanSATE {rel_m:.3e} MeanITE {rel_i:.3e}")
    assert 1e-12 < rel_m < 1e-6 and rel_i < 1e-6 and v_ok, (rel_m, rel_i, v_ok)
