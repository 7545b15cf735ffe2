"""Weighted averages over new individuals without a GPU (gpslc_predict_new_weighted, `averageNew`): the library's
formulas in NumPy (new_average_restatement.structured: one B*' w, one w' B** w, L G solves) against the dense literal side
(w' mean, w' cov w of new_individuals_restatement.literal and the joint covariance of two levels written densely), inside the
tight bounds of tests/test_gpu_group_weights.py with ||w||_1 over the m weights; and the Python front end's parsing and refusals
through the recorder seam of tests/test_frontend_dispatch.py."""
import numpy as np
import pytest

import cases
import new_average_restatement as na
import new_individuals_restatement as nr
from test_frontend_dispatch import _array, recording

WORST = {}


@pytest.mark.parametrize("m", [1, 5, 129, 300])
@pytest.mark.parametrize("n", [24, 129, 200])
@pytest.mark.parametrize("shape", ["UX", "U", "X", "T"])
def test_structured_against_literal(shape, n, m):
    c = cases.make_case(n, shape, False, S=2, seed=3 + n + m)
    Xn, Un = nr.new_individuals(c, m, seed=m, copies=[(0, n - 1)])
    W = na.weight_set(m, seed=n)
    for form in nr.FORMS:
        for L in (1, 5):
            levels = nr.pairs(form, L)
            for s in range(c["S"]):
                got = na.structured(c, s, Xn, Un, m, form, levels, W)
                ref = na.literal(c, s, Xn, Un, m, form, levels, W)
                na.check([g[None] for g in got], [r[None] for r in ref], W, [c["yScale"][s]], f"{form} L={L} s={s}", worst=WORST)
                assert np.array_equal(got[2], np.transpose(got[2], (1, 0, 2)))
                assert not got[0][:, 5].any() and not got[1][:, 5].any() and not got[2][:, :, 5].any()      # the zero column
    print("worst error / tight bound so far:", WORST)


def test_a_unit_vector_is_that_individual_and_the_joint_diagonal_is_the_variance():
    c = cases.make_case(24, "UX", False, S=2, seed=8)
    m = 5
    Xn, Un = nr.new_individuals(c, m)
    W = na.weight_set(m)
    levels = nr.pairs("contrast", 3)
    mu, var, _ = nr.literal(c, 1, Xn, Un, m, "contrast", levels)
    mean, v, cov = na.literal(c, 1, Xn, Un, m, "contrast", levels, W)
    assert np.allclose(mean[:, 3], mu[m // 2], rtol=1e-12, atol=0) and np.allclose(v[:, 3], var[m // 2], rtol=1e-12, atol=0)
    assert np.array_equal(cov[np.arange(3), np.arange(3)], v)


def test_a_contrast_of_a_level_with_itself_is_zero():
    c = cases.make_case(24, "UX", False, S=2, seed=6)
    m = 4
    Xn, Un = nr.new_individuals(c, m)
    W = na.weight_set(m)
    mean, var, cov = na.structured(c, 0, Xn, Un, m, "contrast", [(0.37, 0.37), (0.6, -0.3)], W)
    assert not mean[0].any() and not cov[0, 1].any() and not cov[1, 0].any()
    assert np.allclose(var[0], na.PN * np.sum(W * W, axis=1), rtol=1e-14, atol=0)


# ---- the front end ------------------------------------------------------------------------------------------------------
CASE = cases.make_case(12, "UX", False, S=2, seed=1)
XN, UN = nr.new_individuals(CASE, 3)


@pytest.fixture(scope="module")
def gp_front():
    import causalgpslc_jl_amd as gp_
    return gp_


def _obj(gp, shape="UX", **kw):
    return cases.gpslc_object(gp, CASE if shape == "UX" else cases.make_case(12, shape, False, S=2, seed=1), **kw)


# predictNew's refusals (tests/test_new_individuals.py), raised by the code averageNew shares with it, and the weights' own
REFUSALS = [
    ("UX", dict(Xnew=XN, like=[0, 1, 2], slope=True, baseline=0.1), "slope=True cannot be combined with baseline="),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], doTs=np.zeros((2, 12))), "needs scalar levels"),
    ("UX", dict(like=[0, 1, 2]), "Xnew= is required"),
    ("UX", dict(Xnew=XN), "exactly one of like= and Unew="),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], Unew=UN), "exactly one of like= and Unew="),
    ("U", dict(Xnew=XN, like=[0, 1, 2]), "Xnew= cannot be given"),
    ("X", dict(Xnew=XN, Unew=UN), "like= / Unew= cannot be given"),
    ("T", dict(Xnew=XN), "Xnew= cannot be given"),
    ("UX", dict(Xnew=XN[:, :2], like=[0, 1, 2]), "Xnew must be an (m, nX) array"),
    ("UX", dict(Xnew=XN, like=[0, 1, 12]), "like must be a vector of training indices"),
    ("UX", dict(Xnew=XN, like=[0, 1]), "Xnew has 3 rows"),
    ("UX", dict(Xnew=XN, Unew=UN[:, :1, :]), "Unew must be an (m, nU, S) array"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], doTs=[0.6, np.inf]), "doTs has a non-finite entry"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], baseline=[0.1, 0.2, 0.3]), "baseline must be a scalar or one value per level"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], weights=np.ones(12) / 12), "weights must be a vector of length n = 3"),     # n of the data
    ("UX", dict(Xnew=XN, like=[0, 1, 2], weights=np.ones((3, 2))), "weights must be a vector of length n = 3"),     # (m, G), not (G, m)
    ("UX", dict(Xnew=XN, like=[0, 1, 2], weights=[1.0, np.nan, 0.0]), "weights has a non-finite entry"),
    ("UX", dict(Xnew=XN, like=[0, 1, 2], weights=np.zeros((2, 3), dtype=bool)), "empty group mask"),
]


@pytest.mark.parametrize("shape,kw,message", REFUSALS)
def test_refusals_come_before_any_library_call(gp_front, shape, kw, message):
    kw = dict(kw)
    doTs = kw.pop("doTs", [0.6, 0.2])
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.averageNew(_obj(gp_front, shape), doTs, **kw)
        assert lib.calls == []
    assert message in str(ei.value)


def test_an_fp32_model_is_refused(gp_front):
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.averageNew(_obj(gp_front, fp32_kernel=True), [0.6], Xnew=XN, like=[0, 1, 2])
        assert lib.calls == []
    assert "fp64" in str(ei.value)


def test_the_c_call_of_an_accepted_request(gp_front):
    g = _obj(gp_front)
    idx = [3, 0, 7]
    W = np.array([[0.5, 0.25, 0.25], [1.0, -1.0, 0.0]])
    with recording(gp_front) as lib:
        mean, var, cov = gp_front.averageNew(g, [0.6, 0.2], Xnew=XN, like=idx, weights=W, baseline=0.1, want_cov=True)
    assert [c[0] for c in lib.calls] == ["gpslc_create", "gpslc_set_data", "gpslc_predict_new_weighted"]
    e = lib.calls[2][1]
    assert (e["S"], e["m"], e["form"], e["L"], e["G"], e["pred_noise"]) == (2, 3, 1, 2, 2, 1e-10)
    assert e["U"] == _array(g.U) and e["uyLS"] == _array(g.uyLS) and e["xyLS"] == _array(g.xyLS)
    assert e["tyLS"] == _array(g.tyLS) and e["yScale"] == _array(g.yScale) and e["yNoise"] == _array(g.yNoise)
    assert e["Xnew"] == _array(np.asfortranarray(XN)) and e["Unew"] == _array(np.asfortranarray(CASE["U"][idx]))
    assert e["doT"] == _array(np.array([0.6, 0.2])) and e["doT_base"] == _array(np.array([0.1, 0.1]))
    assert e["weights"] == _array(W) and e["weights"].startswith("f8[2, 3]/[24, 8]")       # weights[i + m*g]
    assert e["meanW"] == e["varW"] == "f8[2, 2, 2]/[8, 16, 32]" and e["covW"] == "f8[2, 2, 2, 2]/[8, 16, 32, 64]"
    fill = lambda *shape: 1.0 + 0.5 * np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    assert np.array_equal(mean, fill(2, 2, 2)) and np.array_equal(var, fill(2, 2, 2)) and np.array_equal(cov, fill(2, 2, 2, 2))


def test_weights_forms_and_the_group_axis(gp_front):
    with recording(gp_front) as lib:
        out = gp_front.averageNew(_obj(gp_front), 0.6, Xnew=XN, Unew=UN, slope=True)                      # 1/m, no group axis
        assert len(out) == 2 and out[0].shape == out[1].shape == (2, 1)
        out = gp_front.averageNew(_obj(gp_front, "T"), [0.6, 0.1, 0.2], want_cov=True)                    # m = 1
        assert out[0].shape == (2, 3) and out[2].shape == (2, 3, 3)
        keys, Wg = gp_front.groupWeights(["a", "b", "a"])
        out = gp_front.averageNew(_obj(gp_front), [0.6, 0.2], Xnew=XN, like=[0, 1, 2], weights=Wg)
        assert out[0].shape == (2, 2, 2)
        out = gp_front.averageNew(_obj(gp_front), [0.6], Xnew=XN, like=[0, 1, 2], weights=[np.array([True, False, True]), np.array([0.0, 1.0, 0.0])])
        assert out[0].shape == (2, 1, 2)
    new = [c[1] for c in lib.calls if c[0] == "gpslc_predict_new_weighted"]
    assert (new[0]["form"], new[0]["L"], new[0]["G"], new[0]["doT_base"], new[0]["covW"]) == (2, 1, 1, None, None)
    assert new[0]["weights"] == _array(np.full((1, 3), 1.0 / 3))
    assert (new[1]["form"], new[1]["m"], new[1]["G"], new[1]["Xnew"], new[1]["Unew"]) == (0, 1, 1, None, None)
    assert new[1]["weights"] == _array(np.ones((1, 1)))
    assert new[2]["weights"] == _array(np.array([[0.5, 0.0, 0.5], [0.0, 1.0, 0.0]]))
    assert new[3]["weights"] == _array(np.array([[0.5, 0.0, 0.5], [0.0, 1.0, 0.0]]))
    assert not any(c[0] == "gpslc_predict_new" for c in lib.calls)
