"""Gradient of the outcome log-likelihood on the GPU (gpslc_y_logpdf_grad) against the host restatement
(grad_restatement.py, long double).

Bound, per posterior sample and output element: tol * scale with tol = max(1e-10, 1e-14 cond(A)) — test_gpu_loo.py's bound — and
the element's error scale from the restatement (the same sum without cancellation).  tests/test_logpdf_grad.py shows on the CPU
that the restatement's own fp64 rounding stays below 1e-3 of that bound, that its closed form matches central differences, and
that these inputs see a missing column sum or an unmasked padding.  Every comparison prints the device's error as a fraction of
the bound."""
import functools

import numpy as np
import pytest

import cases
import grad_restatement as gr
from new_individuals_widths import normalise
from test_gpu_loo import _forced_schedules, _ill_case

pytestmark = pytest.mark.gpu

S = 3


@functools.lru_cache(maxsize=None)
def _case(n, shape, binary_t, S, seed, nU=2, nX=3, normalised=False):
    c = cases.make_case(n, shape, binary_t, S=S, seed=seed, nU=nU, nX=nX)
    return normalise(c) if normalised else c


@functools.lru_cache(maxsize=None)
def _expected(key, samples=None):
    return gr.expected(_case(*key), samples=samples)


def _check(exp, out, samples=None, what=""):
    """out = yLogpdfGrad's dict against exp[s] (grad_restatement.expected): every element within the sample's tol * scale"""
    worst = 0.0
    for s in (exp if samples is None else samples):
        e = exp[s]
        err = gr.errors(gr.device_sample(out, s), e["grads"], e["scales"])
        frac = {k: v / e["tol"] for k, v in err.items()}
        print(what, "sample", s, "cond %.3g tol %.3g" % (e["cond"], e["tol"]), "device error / bound:",
              {k: "%.2e" % v for k, v in frac.items()})
        assert max(frac.values()) <= 1.0, (what, s, frac)
        worst = max(worst, max(frac.values()))
    return worst


def _same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


GRID = ([(200, sh, False) for sh in ("UX", "U", "X", "T")] + [(n, "UX", False) for n in (3, 128, 129, 300)]
        + [(129, "UX", True), (129, "T", False)])


@pytest.mark.parametrize("n,shape,binary_t", GRID)
def test_gradient_against_restatement(gp, n, shape, binary_t):
    """the four model shapes at n = 200; one padded tile, an exact tile, one live row in a second tile, three tiles (off-diagonal
    items with K ranges of 1 and 2); binary and continuous T at n = 129; F = 1 (no U, no X) at n = 129"""
    key = (n, shape, binary_t, S, 140 + n)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    out = gp.yLogpdfGrad(g)
    nU, nX = g.getNU(), g.getNX()
    assert out["dU"].shape == (n, nU, S) and out["duyLS"].shape == (nU, S) and out["dxyLS"].shape == (nX, S)
    assert out["dY"].shape == (n, S) and all(out[k].shape == (S,) for k in ("dtyLS", "dyScale", "dyNoise", "logpdf"))
    _check(_expected(key), out, what=f"n={n} {shape} bin={binary_t}")
    assert not g.ctx().last_info(S).any()


def test_widest_feature_block(gp):
    """nU = 5, nX = 27: F = 33, the widest block the library takes, at n = 129; lengthscales rescaled to sum 1 / l^2 = 0.5 so that
    K is not the identity"""
    key = (129, "UX", False, S, 141, 5, 27, True)
    out = gp.yLogpdfGrad(cases.gpslc_object(gp, _case(*key)))
    _check(_expected(key), out, what="F=33")


def test_ill_conditioned_case(gp):
    c = _ill_case()
    exp = gr.expected(c)
    for s in exp:
        assert 1e4 <= exp[s]["cond"] <= 1e8, exp[s]["cond"]
    _check(exp, gp.yLogpdfGrad(cases.gpslc_object(gp, c)), what="ill-conditioned")


def test_schedules_give_the_same_bits(gp):
    """five tiles, S = 2: the factor and alpha from the persistent launch against the per-column schedule's"""
    c = _case(640, "UX", False, 2, 177)
    out = _forced_schedules(gp, c, lambda g: gp.yLogpdfGrad(g))
    _same_bits(*out, what="schedules")
    assert all(np.isfinite(v).all() for v in out[0].values())


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    key = (300, "UX", False, 5, 178)
    c = _case(*key)
    ref = gp.yLogpdfGrad(cases.gpslc_object(gp, c))
    for tuning in (dict(max_batch=2), dict(n_streams=1), dict(n_streams=3), dict(max_batch=2, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            _same_bits(ref, gp.yLogpdfGrad(g), what=(tuning, rep))
    _check(_expected(key, samples=(1, 4)), ref, what="chunking")


def test_each_output_alone_and_logpdf_of_y_loo(gp):
    c = _case(200, "UX", False, S, 140 + 200)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    args = (S, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    st, full = ctx.y_logpdf_grad(*args)
    assert st == 0
    for name in ctx.GRAD_OUTPUTS[:-1]:
        for want in ((name,), (name, "logpdf")):
            st, one = ctx.y_logpdf_grad(*args, want=want)
            assert st == 0
            for k in ctx.GRAD_OUTPUTS:
                assert (one[k] is None) == (k not in want)
                assert one[k] is None or np.array_equal(one[k], full[k]), (want, k)
    st, _, _, _, logpdf = ctx.y_loo(*args, want=("logpdf",))
    assert st == 0 and np.array_equal(logpdf, full["logpdf"])
    st, only = ctx.y_logpdf_grad(*args, want=("dyScale", "dyNoise", "dY"))      # no pair pass
    assert st == 0 and all(np.array_equal(only[k], full[k]) for k in ("dyScale", "dyNoise", "dY"))


def test_shifting_a_column_of_u_leaves_the_likelihood(gp):
    """sum_i dU[i, f, s] vanishes to the bound (the sum of the elements' bounds)"""
    for key in ((129, "UX", False, S, 140 + 129), (300, "UX", False, S, 140 + 300)):
        out = gp.yLogpdfGrad(cases.gpslc_object(gp, _case(*key)))
        exp = _expected(key)
        for s in range(S):
            total, bound = np.abs(out["dU"][:, :, s].sum(0)), exp[s]["tol"] * np.asarray(exp[s]["scales"]["dU"], dtype=float).sum(0)
            print("n", key[0], "sample", s, "sum dU / bound", total / bound)
            assert np.all(total <= bound)


def test_overrides_against_restatement(gp):
    key = (200, "UX", False, S, 140 + 200)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    rng = np.random.default_rng(5)
    Y2 = rng.standard_normal(200) * 2.0 + 1.0
    X2 = c["X"] + 0.3 * rng.standard_normal(c["X"].shape)
    _check(gr.expected(c, Y=Y2), gp.yLogpdfGrad(g, Y_override=Y2), what="Y override")
    _check(gr.expected(c, X=X2), gp.yLogpdfGrad(g, X_override=X2), what="X override")
    _check(gr.expected(c, X=X2, Y=Y2), gp.yLogpdfGrad(g, X_override=X2, Y_override=Y2), what="both overrides")
    plain = gp.yLogpdfGrad(g)                   # the context's own data afterwards: nothing of the overrides is kept
    _check(_expected(key), plain, what="after the overrides")


@pytest.mark.parametrize("shape", ["UX", "U", "X", "T"])
def test_log_parameters_on_every_model_shape(gp, shape):
    """log_params=True multiplies the five positive parameters' gradients by the parameter; a model without U (without X) keeps
    the empty block of its shape"""
    n = 200
    c = _case(n, shape, False, S, 140 + n)
    g = cases.gpslc_object(gp, c)
    nU, nX = g.getNU(), g.getNX()
    plain, logs = gp.yLogpdfGrad(g), gp.yLogpdfGrad(g, log_params=True)
    assert plain.keys() == logs.keys()
    for k in plain:
        assert logs[k].shape == plain[k].shape, k
    assert logs["duyLS"].shape == (nU, S) and logs["dxyLS"].shape == (nX, S) and logs["dU"].shape == (n, nU, S)
    for k, par in (("duyLS", c["uyLS"]), ("dxyLS", c["xyLS"]), ("dtyLS", c["tyLS"]), ("dyScale", c["yScale"]), ("dyNoise", c["yNoise"])):
        if par is None:
            assert logs[k].size == 0, k
        else:
            assert logs[k].size and np.array_equal(logs[k], plain[k] * par), k
    for k in ("dU", "dY", "logpdf"):
        assert np.array_equal(logs[k], plain[k]), k


def test_breakdown_gives_nan_for_that_sample_only(gp):
    """test_gpu_loo's breakdown: yNoise = 0 and a duplicated individual in a model without U and X — sample 0's matrix is singular
    (pivot 2 is exactly 0); an ordinary error return"""
    c = dict(cases.make_case(200, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    st, out = g.ctx().y_logpdf_grad(2, None, None, None, None, None, g.tyLS, g.yScale, g.yNoise)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for k in ("dtyLS", "dyScale", "dyNoise"):
        assert np.isnan(out[k][0]) and np.isfinite(out[k][1]), k
    assert np.isnan(out["dY"][:, 0]).all()
    _check(gr.expected(c, samples=(1,)), out, what="beside a breakdown")
    with pytest.raises(gp.PosDefException) as ei:
        gp.yLogpdfGrad(g)
    assert ei.value.info == 2


def test_breakdown_with_u_and_x(gp):
    """the same breakdown in a model with U and X — individual 1 copies individual 0 in U (sample 0), X and T, yNoise = 0, yScale =
    1: pivot 2 is exactly 0 — so that the pair pass runs over that sample's W and grad_finish_kernel writes NaN into dU, duyLS
    and dxyLS of that sample only"""
    c = dict(cases.make_case(200, "UX", False, S=2, seed=184))
    for k in ("T", "X", "U"):
        c[k] = c[k].copy(order="F")
    c["T"][1], c["X"][1], c["U"][1, :, 0] = c["T"][0], c["X"][0], c["U"][0, :, 0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    st, out = g.ctx().y_logpdf_grad(2, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    assert np.isnan(out["dU"][:, :, 0]).all() and np.isnan(out["dY"][:, 0]).all()
    for k in ("duyLS", "dxyLS"):
        assert np.isnan(out[k][:, 0]).all() and np.isfinite(out[k][:, 1]).all(), k
    for k in ("dtyLS", "dyScale", "dyNoise"):
        assert np.isnan(out[k][0]) and np.isfinite(out[k][1]), k
    assert np.isfinite(out["dU"][:, :, 1]).all()
    _check(gr.expected(c, samples=(1,)), out, what="beside a breakdown, UX")


def test_argument_errors(gp):
    c = _case(24, "UX", False, 2, 186)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    args = (g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    assert ctx.y_logpdf_grad(2, *args, want=())[0] == -11               # every gradient output NULL: dU's position
    assert ctx.y_logpdf_grad(2, *args, want=("logpdf",))[0] == -11      # logpdf alone is gpslc_y_logpdf's call
    assert b"NULL" in ctx.lib.gpslc_last_error(ctx.h)
    assert ctx.y_logpdf_grad(-1, *args)[0] == -2                        # S < 0
    assert ctx.y_logpdf_grad(2, None, *args[1:])[0] == -3               # U missing with nU > 0
    st, out = ctx.y_logpdf_grad(0, *args)                               # an empty call
    assert st == 0 and out["dU"].shape == (24, 2, 0) and out["dY"].shape == (24, 0)
    f32 = cases.gpslc_object(gp, c, fp32_kernel=True)
    assert f32.ctx().y_logpdf_grad(2, *args)[0] == -1007                # GPSLC_ERR_UNSUPPORTED
    assert b"fp64" in f32.ctx().lib.gpslc_last_error(f32.ctx().h)
    with pytest.raises(gp.GPSLCError):
        gp.yLogpdfGrad(f32)
    assert ctx.y_logpdf_grad(2, *args)[0] == 0                          # and the good call still runs
