"""Unit invariance (tests/test_gpu_offscale.py, a and b) for the entry points added after it: the slope and outcome forms of
`predict` and `ITEDistributions`, `predictNew`, `looPredictive` and `lgoPredictive`.  The transforms, the exponents and the bit
comparison are that module's (tests/offscale.py); new individuals are rescaled column for column like the training data.

  1. powers of two on every feature column and its lengthscale: no bit of any output moves;
  2. the same with T, tyLS and the levels times 2**E_T: outputs that are values of the surface still do not move; a slope is a
     derivative in T's unit — its means come out times 2**-E_T and its variances and covariances times 4**-E_T, exactly, with the
     jitter that is added to them scaled alike (predictionCovarianceNoise through HyperParameters, pred_noise through the
     C-level Context.predict_new);
  3. the outcome's unit, Y by 2**k with yScale, yNoise and the jitter by 4**k: means times 2**k, variances and covariances times
     4**k, exactly; looLpd and lgoLpd hold a logarithm and are compared with the restatement of the rescaled case at the bounds
     of tests/test_gpu_loo.py and tests/test_gpu_lgo.py."""
import functools

import numpy as np
import pytest

import cases
import lgo_restatement as lg
import loo_restatement as lr
import new_individuals_restatement as nr
import offscale
from test_gpu_lgo import _check as _check_lgo
from test_gpu_loo import _check as _check_loo
from test_gpu_offscale import E_T, E_U, E_X, _same

pytestmark = pytest.mark.gpu

CASES = [(129, "UX", False), (200, "X", False), (200, "U", False), (129, "T", False)]
M = 130                                            # two row tiles of new individuals
PN = nr.PN
FIRST = ("mean", "meanSATE", "MeanITE")          # outputs of the first order in the scaled unit; var, varSATE, cov: second
LPD = ("loo.lpd", "lgo.lpd")


@functools.lru_cache(maxsize=None)
def _case(n, shape, bt):
    c = cases.make_case(n, shape, bt, S=3, seed=870 + n + 7 * list(cases.SHAPES).index(shape))
    Xn, Un = nr.new_individuals(c, M, seed=n)
    return dict(c, baseline=np.array([0.9, -0.2]), sweep=np.linspace(-0.7, 0.9, 5)), Xn, Un


def _rescale_new(Xn, Un):
    return (None if Xn is None else np.asfortranarray(Xn * np.ldexp(1.0, np.array(E_X))[None, :]),
            None if Un is None else np.asfortranarray(Un * np.ldexp(1.0, np.array(E_U))[None, :, None]))


def _outputs(gp, c, Xn, Un, pn=PN, pn_slope=None):
    """name -> array: every entry point added since tests/test_gpu_offscale.py on one object of the case; the slope outputs, whose
    jitter has another unit once T is rescaled, from an object with `pn_slope`"""
    pn_slope = pn if pn_slope is None else pn_slope
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn))
    gs = g if pn_slope == pn else cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn_slope))
    out = {}

    def put(prefix, names, arrays):
        for k, a in zip(names, arrays):
            out[f"{prefix}.{k}"] = a

    def new(obj, form, doT, base, noise):
        st, *arrays = obj.ctx().predict_new(3, obj.U, obj.uyLS, obj.xyLS, obj.tyLS, obj.yScale, obj.yNoise, M, Xn, Un, form, doT,
                                            base, noise, want=("mean", "var", "cov"))
        assert st == 0
        return arrays
    three = ("meanSATE", "varSATE", "MeanITE")
    put("loo", ("mean", "var", "lpd"), gp.looPredictive(g))
    put("lgo", ("mean", "var", "lpd"), gp.lgoPredictive(g, groups=lg.mod7(c["n"]))[:3])
    put("new.outcome", ("mean", "var", "cov"), new(g, "outcome", c["sweep"], None, pn))
    put("new.contrast", ("mean", "var", "cov"), new(g, "contrast", c["doTs"], c["baseline"], pn))
    put("outcome.L2", three, gp.predict(g, c["doTs"], want_mean_ite=True, outcome=True))
    put("outcome.L5", three, gp.predict(g, c["sweep"], want_mean_ite=True, outcome=True))
    put("outcome.itedist", ("mean", "cov"), gp.ITEDistributions(g, float(c["doTs"][1]), outcome=True))
    put("slope.L2", three, gp.predict(gs, c["doTs"], want_mean_ite=True, slope=True))
    put("slope.L5", three, gp.predict(gs, c["sweep"], want_mean_ite=True, slope=True))
    put("slope.itedist", ("mean", "cov"), gp.ITEDistributions(gs, float(c["doTs"][1]), slope=True))
    put("slope.new", ("mean", "var", "cov"), new(gs, "slope", c["sweep"], None, pn_slope))
    for o in {id(g): g, id(gs): gs}.values():
        o.ctx().close()
    assert len(out) == 31 and all(np.all(np.isfinite(a)) for a in out.values())
    return out


@functools.lru_cache(maxsize=None)
def _plain(gp, n, shape, bt):
    """the plain case's outputs, computed once and left unchanged"""
    return _outputs(gp, *_case(n, shape, bt))


def _order(name):
    return 1 if name.rsplit(".", 1)[1] in FIRST else 2


@pytest.mark.parametrize("n,shape,bt", CASES)
def test_a_change_of_the_features_units_moves_no_bit(gp, n, shape, bt):
    c, Xn, Un = _case(n, shape, bt)
    plain = _plain(gp, n, shape, bt)
    scaled = _outputs(gp, offscale.rescale_features(c, E_X, E_U, 0), *_rescale_new(Xn, Un))
    assert sorted(plain) == sorted(scaled)
    for k in plain:
        _same(k, scaled[k], plain[k])


@pytest.mark.parametrize("n,shape,bt", CASES)
def test_a_change_of_the_treatments_unit_scales_the_slopes_only(gp, n, shape, bt):
    """T, tyLS and every level times 2**E_T beside the feature columns: (d d) wt keeps every bit, so every value of the surface
    does; the slope's cross factor 2 (T_j - a) r wt and its prior 2 wt are products of exact powers of two of the unit"""
    c, Xn, Un = _case(n, shape, bt)
    plain = _plain(gp, n, shape, bt)
    scaled = _outputs(gp, offscale.rescale_features(c, E_X, E_U, E_T), *_rescale_new(Xn, Un), pn_slope=PN * 4.0 ** -E_T)
    for k in plain:
        f = 2.0 ** (-E_T * _order(k)) if k.startswith("slope.") else 1.0
        _same(k, scaled[k], plain[k] * f)


@pytest.mark.parametrize("k", [-9, 11])
@pytest.mark.parametrize("n,shape,bt", CASES)
def test_the_outcomes_unit_scales_the_newer_outputs_by_an_exact_power_of_two(gp, n, shape, bt, k):
    c, Xn, Un = _case(n, shape, bt)
    r = offscale.rescale_outcome(c, k)
    plain = _plain(gp, n, shape, bt)
    scaled = _outputs(gp, r, Xn, Un, pn=PN * 4.0 ** k)
    for name in plain:
        if name not in LPD:
            _same(name, scaled[name], plain[name] * 2.0 ** (k * _order(name)))
    labels = lg.mod7(n)
    _check_loo(lr.expected(r, samples=(1,)), tuple(scaled[f"loo.{x}"] for x in ("mean", "var", "lpd")), r["Y"], what=f"loo k={k}")
    _check_lgo(lg.expected(r, labels, samples=(1,)), tuple(scaled[f"lgo.{x}"] for x in ("mean", "var", "lpd")), r["Y"], labels,
               what=f"lgo k={k}")
