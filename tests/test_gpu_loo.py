"""Leave-one-out predictive checks on the GPU (gpslc_y_loo) against the host restatement (loo_restatement.py).

Bound, per posterior sample: tol = max(1e-10, 1e-14 cond(A)) — 1e-10 is test_gpu_estimation's bound for y_logpdf against the
oracle, the cond term follows cases.draw_bounds.  looVar relative, looMean absolute against tol max|Y|, looLpd absolute against
tol (1 + max_i zscore_i^2).  Every comparison first asserts that the restatement's two computations (closed form, literal refit)
agree within the same bound; the device is then compared with the literal refit."""
import functools

import numpy as np
import pytest

import cases
import loo_restatement as lr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(n, shape, binary_t, S, seed):
    return cases.make_case(n, shape, binary_t, S=S, seed=seed)


@functools.lru_cache(maxsize=None)
def _expected(n, shape, binary_t, S, seed, samples=None):
    return lr.expected(_case(n, shape, binary_t, S, seed), samples=samples)


def _check(exp, got, Y, samples=None, tol=None, what=""):
    """got = (mean, var, lpd) (n, S) against exp[s]; tol=None: the sample's own bound"""
    for s in (exp if samples is None else samples):
        e = exp[s]
        t = e["tol"] if tol is None else tol
        host = lr.errors(e["closed"], e["refit"], Y)
        dev = lr.errors(tuple(a[:, s] for a in got), e["refit"], Y)
        print(what, "sample", s, "cond %.3g tol %.3g" % (e["cond"], t), "host (var, mean, lpd)", host, "device", dev)
        assert max(host) <= (e["tol"] if tol is None else min(tol, e["tol"])), ("host", s, host)
        assert max(dev) <= t, ("device", s, dev)


GRID = [(n, "UX") for n in (1, 3, 128, 129, 200, 400)] + [(200, sh) for sh in ("U", "X", "T")]


@pytest.mark.parametrize("binary_t", [False, True])
@pytest.mark.parametrize("n,shape", GRID)
def test_loo_against_restatement(gp, n, shape, binary_t):
    """one tile with padding, an exact tile, one live row in a second tile, four tiles (row chains of lengths 1 to 4); all four
    model shapes at n = 200"""
    key = (n, shape, binary_t, 2, 40 + n)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    got = gp.looPredictive(g)
    assert all(a.shape == (n, 2) for a in got)
    _check(_expected(*key), got, c["Y"], what=f"n={n} {shape} bin={binary_t}")
    assert not g.ctx().last_info(2).any()


def _forced_schedules(gp, c, run):
    """`run(g)` under the persistent task launch forced down to one matrix and under the per-column schedule (as
    test_gpu_outcome.py does): the two outputs, after checking with the HIP-event records which schedule really ran."""
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


def test_schedules_give_the_same_bits(gp):
    """five tiles, S = 5: alpha from the persistent launch's last task against launch_backsolve's, the factor from either"""
    key = (520, "UX", False, 5, 77)
    c = _case(*key)
    out = _forced_schedules(gp, c, lambda g: gp.looPredictive(g))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    _check(_expected(*key, samples=(0, 4)), out[0], c["Y"], what="schedules")


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    key = (300, "UX", False, 5, 78)
    c = _case(*key)
    ref = gp.looPredictive(cases.gpslc_object(gp, c))
    for tuning in (dict(max_batch=2), dict(n_streams=1), dict(n_streams=3), dict(max_batch=2, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            for x, y in zip(ref, gp.looPredictive(g)):
                assert np.array_equal(x, y), (tuning, rep)
    _check(_expected(*key, samples=(1,)), ref, c["Y"], what="chunking")


@pytest.mark.parametrize("n,fp32", [(700, False), (200, True)])
def test_logpdf_comes_from_the_same_factorisation(gp, n, fp32):
    """logpdf_or_null is gpslc_y_logpdf's value bit for bit wherever that call takes the batched tiled path (n > 640; an fp32
    context at any n)"""
    c = _case(n, "UX", False, 2, 79)
    g = cases.gpslc_object(gp, c, fp32_kernel=fp32)
    st, mean, var, lpd, logpdf = g.ctx().y_loo(2, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    assert st == 0
    assert np.array_equal(logpdf, gp.yLogpdf(g))
    assert np.isfinite(mean).all() and (var > 0).all() and np.isfinite(lpd).all()


def test_logpdf_at_a_size_where_y_logpdf_runs_in_one_workgroup(gp):
    """n = 200: gpslc_y_logpdf scores in a single workgroup, gpslc_y_loo on the tiled path — the same number to test_gpu_estimation's
    bound for y_logpdf"""
    c = _case(200, "UX", False, 2, 40 + 200)
    g = cases.gpslc_object(gp, c)
    st, _, _, _, logpdf = g.ctx().y_loo(2, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, want=("logpdf",))
    assert st == 0
    assert np.allclose(logpdf, gp.yLogpdf(g), rtol=1e-10, atol=1e-9)


def test_each_output_alone(gp):
    c = _case(200, "UX", False, 2, 40 + 200)
    g = cases.gpslc_object(gp, c)
    args = (2, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    full = g.ctx().y_loo(*args)
    assert full[0] == 0
    for k, name in enumerate(("mean", "var", "lpd", "logpdf"), start=1):
        one = g.ctx().y_loo(*args, want=(name,))
        assert one[0] == 0
        for j in range(1, 5):
            assert (one[j] is None) == (j != k)
        assert np.array_equal(one[k], full[k]), name


def test_overrides_against_restatement(gp):
    key = (200, "UX", False, 2, 40 + 200)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    rng = np.random.default_rng(5)
    Y2 = rng.standard_normal(200) * 2.0 + 1.0
    X2 = c["X"] + 0.3 * rng.standard_normal(c["X"].shape)
    _check(lr.expected(c, Y=Y2), gp.looPredictive(g, Y_override=Y2), Y2, what="Y override")
    _check(lr.expected(c, X=X2), gp.looPredictive(g, X_override=X2), c["Y"], what="X override")
    _check(lr.expected(c, X=X2, Y=Y2), gp.looPredictive(g, X_override=X2, Y_override=Y2), Y2, what="both overrides")
    # the context's own data afterwards: nothing of the overrides is kept
    _check(_expected(*key), gp.looPredictive(g), c["Y"], what="after the overrides")
    s = gp.looSummary(g, Y_override=Y2)
    m, v, l = gp.looPredictive(g, Y_override=Y2)
    assert np.array_equal(s["zscore"], (Y2[:, None] - m) / np.sqrt(v)) and np.array_equal(s["elpd"], l.sum(axis=0))


def test_scaling_y_scales_the_mean_and_leaves_the_variance(gp):
    key = (200, "UX", False, 2, 40 + 200)
    c = _case(*key)
    exp = _expected(*key)
    g = cases.gpslc_object(gp, c)
    m1, v1, _ = gp.looPredictive(g)
    m3, v3, _ = gp.looPredictive(g, Y_override=3.0 * c["Y"])
    for s in range(2):
        tol = exp[s]["tol"]
        assert np.max(np.abs(m3[:, s] - 3.0 * m1[:, s])) <= tol * 3.0 * np.max(np.abs(c["Y"]))
        assert np.max(np.abs(v3[:, s] - v1[:, s]) / v1[:, s]) <= tol


def _ill_case():
    """n = 200 with long lengthscales and a small yNoise: A is close to a low-rank matrix plus yNoise I"""
    c = dict(cases.make_case(200, "UX", False, S=2, seed=83))
    c["uyLS"] = np.asfortranarray(np.full_like(c["uyLS"], 6.0))
    c["xyLS"] = np.asfortranarray(np.full_like(c["xyLS"], 8.0))
    c["tyLS"] = np.array([5.0, 7.0])
    c["yScale"] = np.array([1.0, 2.0])
    c["yNoise"] = np.array([1e-3, 2e-4])
    return c


def test_ill_conditioned_case(gp):
    c = _ill_case()
    exp = lr.expected(c)
    for s in exp:
        assert 1e4 <= exp[s]["cond"] <= 1e8, exp[s]["cond"]
    _check(exp, gp.looPredictive(cases.gpslc_object(gp, c)), c["Y"], what="ill-conditioned")


def test_breakdown_gives_nan_for_that_sample_only(gp):
    """yNoise = 0 and a duplicated individual in a model without U and X: sample 0's matrix is singular (pivot 2 is exactly 0);
    an ordinary error return"""
    c = dict(cases.make_case(200, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    st, mean, var, lpd, logpdf = g.ctx().y_loo(2, None, None, None, None, None, g.tyLS, g.yScale, g.yNoise)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for a in (mean, var, lpd):
        assert np.isnan(a[:, 0]).all()
    _check(lr.expected(c, samples=(1,)), (mean, var, lpd), c["Y"], what="beside a breakdown")
    with pytest.raises(gp.PosDefException) as ei:
        gp.looPredictive(g)
    assert ei.value.info == 2
    with pytest.raises(gp.PosDefException) as ei:
        gp.yLogpdf(g)                                   # the same pivot from gpslc_y_logpdf
    assert ei.value.info == 2
    # the context keeps working
    c["yNoise"] = np.array([c["yNoise"][1], c["yNoise"][1]])
    g2 = cases.gpslc_object(gp, c)
    g2._ctx = g.ctx()
    assert np.isfinite(np.stack(gp.looPredictive(g2))).all()


def test_fp32_context_against_the_fp64_restatement(gp):
    """the bound of test_fp32_kernel_mode_drift_and_identities: 1e-6, relative for looVar and scaled as above for the others"""
    key = (300, "UX", False, 2, 85)
    c = _case(*key)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    _check(_expected(*key), gp.looPredictive(g), c["Y"], tol=1e-6, what="fp32")


def test_argument_errors(gp):
    c = _case(24, "UX", False, 2, 86)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    args = (g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    assert ctx.y_loo(2, *args, want=())[0] == -11                    # all four outputs NULL: looMean's position
    assert b"NULL" in ctx.lib.gpslc_last_error(ctx.h)
    assert ctx.y_loo(-1, *args)[0] == -2                             # S < 0
    assert ctx.y_loo(2, None, *args[1:])[0] == -3                    # U missing with nU > 0
    assert ctx.y_loo(2, *args[:5], None, *args[6:])[0] == -6         # tyLS missing: gpslc_y_logpdf's numbering
    st, mean, var, lpd, logpdf = ctx.y_loo(0, *args)                 # an empty call
    assert st == 0 and mean.shape == (24, 0)
    fresh = gp.Context(24, 3, 2)
    assert fresh.y_loo(2, *args)[0] == -1002                         # GPSLC_ERR_NODATA: before set_data
    with pytest.raises(gp.GPSLCError) as ei:
        fresh.check(fresh.y_loo(2, *args)[0])
    assert "set_data" in str(ei.value)
    assert ctx.y_loo(2, *args)[0] == 0                               # and the good call still runs
