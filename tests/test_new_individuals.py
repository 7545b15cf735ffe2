"""Predictions for new individuals without a GPU: the restatement's two sides against an extended-precision computation, and the
Python front end's refusals and marshalling through the recorder seam of tests/test_frontend_dispatch.py.

Bounds (the tight ones of test_gpu_contrast._check, which tests/test_gpu_new_individuals.py applies to the device): means within
1e-9 max|ref| + 1e-13, variances and covariances within 1e-9 |ref| + 1e-12 yScale, |ref| of a covariance block its largest entry.
The reference is `structured` in np.longdouble (kernel values, a Cholesky written out in NumPy, substitutions)."""
import numpy as np
import pytest

import cases
import new_individuals_restatement as nr
from test_frontend_dispatch import _array, recording

# (shape, binary T, n, m, L, form): every model shape and form, a second row tile with one live row, more new individuals than
# training individuals, and in each case new individuals 0 and 1 as exact copies of training individuals
GRID = [("UX", False, 24, 3, 2, "outcome"), ("U", False, 129, 5, 2, "contrast"), ("X", True, 24, 40, 2, "slope"),
        ("T", False, 40, 3, 2, "contrast"), ("UX", True, 60, 129, 1, "outcome"), ("X", False, 129, 5, 3, "slope"),
        ("U", True, 24, 30, 2, "contrast"), ("T", True, 24, 2, 2, "outcome")]


def _close(got, ref, ys, what, mean=False):
    ref = np.asarray(ref)
    scale = float(np.max(np.abs(ref))) if (mean or ref.ndim == 2) else np.abs(ref).astype(np.float64)
    bound = 1e-9 * scale + (1e-13 if mean else 1e-12 * ys)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref).astype(np.float64)
    print(what, "max err / bound", float(np.max(err / bound)))
    assert np.all(err <= bound), what


@pytest.mark.parametrize("shape,bt,n,m,L,form", GRID)
def test_both_restatements_against_extended_precision(shape, bt, n, m, L, form):
    assert np.finfo(np.longdouble).eps < 1e-18
    c = cases.make_case(n, shape, bt, S=2, seed=11 + n + m)
    Xn, Un = nr.new_individuals(c, m, seed=m, copies=[(0, n - 1), (1, 2)][:m])
    levels = nr.pairs(form, L)
    for s in range(c["S"]):
        ys = float(c["yScale"][s])
        ref = nr.structured(c, s, Xn, Un, m, form, levels, dtype=np.longdouble)
        for name, got in (("literal", nr.literal(c, s, Xn, Un, m, form, levels)),
                          ("structured", nr.structured(c, s, Xn, Un, m, form, levels))):
            for l in range(L):
                what = f"{name} s={s} l={l}"
                _close(got[0][:, l], ref[0][:, l], ys, what + " mean", mean=True)
                _close(got[1][:, l], ref[1][:, l], ys, what + " var")
                _close(got[2][l], ref[2][l], ys, what + " cov")
                _close(np.diag(got[2][l]), ref[1][:, l], ys, what + " diag(cov) against var")


def test_a_copy_of_a_training_individual_reproduces_its_row():
    """new individual 0 copies training individual n - 1: the restatement of the outcome at new individuals gives the training
    individual's entry of outcome_restatement's dense CovC22 path"""
    import outcome_restatement as outr
    c = cases.make_case(24, "UX", False, S=2, seed=5)
    idx = [23, 2, 7]
    Xn, Un = nr.new_individuals(c, 3, copies=list(enumerate(idx)))
    exp = outr.expected_outcome(c, [0.6, -0.4])
    got = nr.expected(c, Xn, Un, 3, "outcome", [(0.6, None), (-0.4, None)])
    for s in range(2):
        for l in range(2):
            assert np.allclose(got["mean"][:, s, l], exp["meanITE"][idx, s, l], rtol=1e-9, atol=1e-12)
            assert np.allclose(got["cov"][s, l], exp["covITE"][s, l][np.ix_(idx, idx)], rtol=1e-9, atol=1e-12 * c["yScale"][s])


def test_a_contrast_of_a_level_with_itself_is_zero():
    c = cases.make_case(24, "UX", False, S=2, seed=6)
    Xn, Un = nr.new_individuals(c, 4)
    mean, var, cov = nr.structured(c, 0, Xn, Un, 4, "contrast", [(0.37, 0.37)])
    assert not mean.any() and np.array_equal(var, np.full((4, 1), nr.PN)) and np.array_equal(cov[0], nr.PN * np.eye(4))


# ---- the front end ------------------------------------------------------------------------------------------------------
CASE = cases.make_case(12, "UX", False, S=2, seed=1)
XN, UN = nr.new_individuals(CASE, 3)


def _obj(gp, shape="UX", **kw):
    return cases.gpslc_object(gp, CASE if shape == "UX" else cases.make_case(12, shape, False, S=2, seed=1), **kw)


REFUSALS = [
    ("UX", dict(Xnew=XN, like=[0, 1, 2], slope=True, baseline=0.1), "slope=True cannot be combined with baseline="),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], doTs=np.zeros((2, 12))), "needs scalar levels"),
    ("UX", dict(like=[0, 1, 2]), "Xnew= is required"),
    ("UX", dict(Xnew=XN), "exactly one of like= and Unew="),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], Unew=UN), "exactly one of like= and Unew="),
    ("U", dict(Xnew=XN, like=[0, 1, 2]), "Xnew= cannot be given"),
    ("X", dict(Xnew=XN, like=[0, 1, 2]), "like= / Unew= cannot be given"),
    ("X", dict(Xnew=XN, Unew=UN), "like= / Unew= cannot be given"),
    ("T", dict(Xnew=XN), "Xnew= cannot be given"),
    ("UX", dict(Xnew=XN[:, :2], like=[0, 1, 2]), "Xnew must be an (m, nX) array"),
    ("UX", dict(Xnew=XN, like=[0, 1, 12]), "like must be a vector of training indices"),
    ("UX", dict(Xnew=XN, like=[0.0, 1.0, 2.0]), "like must be a vector of training indices"),
    ("UX", dict(Xnew=XN, like=[0, 1]), "Xnew has 3 rows"),
    ("UX", dict(Xnew=XN, Unew=UN[:, :1, :]), "Unew must be an (m, nU, S) array"),
    ("UX", dict(Xnew=np.where(np.arange(9).reshape(3, 3) == 4, np.nan, XN), like=[0, 1, 2]), "Xnew has a non-finite entry"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], doTs=[0.6, np.inf]), "doTs has a non-finite entry"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], baseline=[0.1, 0.2, 0.3]), "baseline must be a scalar or one value per level"),
]


@pytest.mark.parametrize("shape,kw,message", REFUSALS)
def test_refusals_come_before_any_library_call(gp_front, shape, kw, message):
    kw = dict(kw)
    doTs = kw.pop("doTs", [0.6, 0.2])
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.predictNew(_obj(gp_front, shape), doTs, **kw)
        assert lib.calls == []
    assert message in str(ei.value)


def test_an_fp32_model_is_refused(gp_front):
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.predictNew(_obj(gp_front, fp32_kernel=True), [0.6], Xnew=XN, like=[0, 1, 2])
        assert lib.calls == []
    assert "fp64" in str(ei.value)


@pytest.fixture(scope="module")
def gp_front():
    import causalgpslc_jl_amd as gp_
    return gp_


def test_the_c_call_of_an_accepted_request(gp_front):
    g = _obj(gp_front)
    idx = [3, 0, 7]
    with recording(gp_front) as lib:
        mean, var, cov = gp_front.predictNew(g, [0.6, 0.2], Xnew=XN, like=idx, baseline=0.1, want_cov=True)
    assert [c[0] for c in lib.calls] == ["gpslc_create", "gpslc_set_data", "gpslc_predict_new"]
    e = lib.calls[2][1]
    assert (e["S"], e["m"], e["form"], e["L"], e["pred_noise"]) == (2, 3, 1, 2, 1e-10)
    assert e["U"] == _array(g.U) and e["uyLS"] == _array(g.uyLS) and e["xyLS"] == _array(g.xyLS)
    assert e["tyLS"] == _array(g.tyLS) and e["yScale"] == _array(g.yScale) and e["yNoise"] == _array(g.yNoise)
    assert e["Xnew"] == _array(np.asfortranarray(XN)) and e["Xnew"].startswith("f8[3, 3]/[8, 24]")
    assert e["Unew"] == _array(np.asfortranarray(CASE["U"][idx])) and e["Unew"].startswith("f8[3, 2, 2]/[8, 24, 48]")
    assert e["doT"] == _array(np.array([0.6, 0.2])) and e["doT_base"] == _array(np.array([0.1, 0.1]))
    assert e["mean"] == e["var"] == "f8[3, 2, 2]/[8, 24, 48]" and e["cov"] == "f8[3, 3, 2, 2]/[8, 24, 72, 144]"
    # what comes back: the recorder filled every output with 1 + index / 2 (C order of its shape)
    fill = lambda *shape: 1.0 + 0.5 * np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    assert np.array_equal(mean, fill(3, 2, 2)) and np.array_equal(var, fill(3, 2, 2))
    assert cov.shape == (2, 2, 3, 3) and np.array_equal(cov, np.transpose(fill(3, 3, 2, 2), (2, 3, 0, 1)))


def test_forms_and_optional_outputs_reach_the_library_as_asked(gp_front):
    with recording(gp_front) as lib:
        out = gp_front.predictNew(_obj(gp_front), 0.6, Xnew=XN, Unew=UN, slope=True, want_var=False)
        assert len(out) == 2 and out[1] is None
        out = gp_front.predictNew(_obj(gp_front, "T"), [0.6, 0.1, 0.2])
        assert out[0].shape == (1, 2, 3)
    new = [c[1] for c in lib.calls if c[0] == "gpslc_predict_new"]
    assert (new[0]["form"], new[0]["L"], new[0]["doT_base"], new[0]["var"], new[0]["cov"]) == (2, 1, None, None, None)
    assert new[0]["Unew"] == _array(np.asfortranarray(UN))
    assert (new[1]["form"], new[1]["m"], new[1]["Xnew"], new[1]["Unew"], new[1]["cov"]) == (0, 1, None, None, None)
