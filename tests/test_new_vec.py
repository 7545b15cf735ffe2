"""New individuals at per-individual levels and the test-set score without a GPU (gpslc_predict_new_vec, gpslc_y_test, DESIGN.md
§29): the restatement of tests/new_vec_restatement.py held against an extended-precision computation on every case the device
tests use, and the Python front end (`predictNew` with 2-D levels and `Tnew=`, `testPredictive`, `testSummary`) through the recorder
seam of tests/test_frontend_dispatch.py.

Bounds.  The device is held to the tight stage of test_gpu_contrast._check: means (and log densities) within 1e-9 max|ref| + 1e-13,
variances and covariances within 1e-9 |ref| + 1e-12 yScale (|ref| of a covariance block its largest entry).  Here both float64 sides
of the restatement must sit within 1e-3 of that against `structured` in np.longdouble, so that the device tests measure the device."""
import numpy as np
import pytest

import new_vec_restatement as nv
import gpslc_oracle as orc
from test_frontend_dispatch import _array, recording
from test_new_individuals import CASE, XN, UN, _obj

LD = np.longdouble
FRAC = 1e-3      # of the device's bound


def bound(ref, ys, mean=False):
    """the tight bound for an output with reference values `ref`"""
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.max(np.abs(ref))) if (mean or ref.ndim == 2) else np.abs(ref)
    return 1e-9 * scale + (1e-13 if mean else 1e-12 * ys)


def _close(got, ref, ys, what, mean=False, frac=FRAC):
    b = frac * bound(ref, ys, mean)
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    print(what, "max err / bound", float(np.max(err / b)))
    assert np.all(err <= b), what


@pytest.mark.parametrize("shape,bt,n,m,L,form,with_cov", nv.GRID)
def test_both_restatements_against_extended_precision(shape, bt, n, m, L, form, with_cov):
    assert np.finfo(LD).eps < 1e-18
    c, Xn, Un, A_, B_ = nv.grid_case(shape, bt, n, m, L, form)
    for s in range(c["S"]):
        ys = float(c["yScale"][s])
        ref = nv.structured(c, s, Xn, Un, m, form, A_, B_, dtype=LD, want_cov=with_cov)
        for name, got in (("literal", nv.literal(c, s, Xn, Un, m, form, A_, B_, want_cov=with_cov)),
                          ("structured", nv.structured(c, s, Xn, Un, m, form, A_, B_, want_cov=with_cov))):
            for l in range(L):
                what = f"{name} s={s} l={l}"
                _close(got[0][:, l], ref[0][:, l], ys, what + " mean", mean=True)
                _close(got[1][:, l], ref[1][:, l], ys, what + " var")
                if with_cov:
                    _close(got[2][l], ref[2][l], ys, what + " cov")
                    _close(np.diag(got[2][l]), ref[1][:, l], ys, what + " diag(cov) against var")


@pytest.mark.parametrize("shape,bt,n,m,L,form,with_cov", [g for g in nv.GRID if g[3] > 1])
def test_the_cases_tell_a_vector_level_from_a_scalar_one(shape, bt, n, m, L, form, with_cov):
    """every new individual at the MEAN dose of its level instead of its own: each output moves by at least 1e6 tight bounds"""
    c, Xn, Un, A_, B_ = nv.grid_case(shape, bt, n, m, L, form)
    flat = lambda V: None if V is None else np.tile(V.mean(axis=0, keepdims=True), (m, 1))
    for s in range(c["S"]):
        ys = float(c["yScale"][s])
        ref = nv.structured(c, s, Xn, Un, m, form, A_, B_, want_cov=with_cov)
        alt = nv.structured(c, s, Xn, Un, m, form, flat(A_), flat(B_), want_cov=with_cov)
        for l in range(L):
            moved = [("mean", np.max(np.abs(alt[0][:, l] - ref[0][:, l])), np.max(bound(ref[0][:, l], ys, mean=True))),
                     ("var", np.max(np.abs(alt[1][:, l] - ref[1][:, l])), np.max(bound(ref[1][:, l], ys)))]
            if with_cov:
                moved.append(("cov", np.max(np.abs(alt[2][l] - ref[2][l])), np.max(bound(ref[2][l], ys))))
            for what, d, b in moved:
                print(f"s={s} l={l} {what} moves by {d:.3e} = {d / b:.3e} bounds")
                assert d >= 1e6 * b, (what, s, l)


@pytest.mark.parametrize("shape,bt,n,m", nv.SCORE_GRID)
def test_the_score_restatement_against_extended_precision(shape, bt, n, m):
    c, Xn, Un, Tt, Yt = nv.score_case(shape, bt, n, m)
    for s in range(c["S"]):
        ys, yn = float(c["yScale"][s]), float(c["yNoise"][s])
        ref = nv.score(c, s, Xn, Un, m, Tt, Yt, "structured", LD)
        # C = (B** o P - W* W*') + yNoise I with 0 <= the bracket (a posterior covariance) <= B** o P, whose trace is m yScale
        cond = np.linalg.cond(np.asarray(ref[4], dtype=np.float64))
        print(f"s={s} cond(C) = {cond:.3e} (m yScale / yNoise + 1 = {m * ys / yn + 1:.3e})")
        assert cond <= (m * ys / yn + 1) * (1 + 1e-6)
        for name, got in (("literal", nv.score(c, s, Xn, Un, m, Tt, Yt)), ("structured", nv.score(c, s, Xn, Un, m, Tt, Yt, "structured"))):
            what = f"{name} s={s}"
            _close(got[0], ref[0], ys, what + " mean", mean=True)
            _close(got[1], ref[1], ys, what + " var")
            _close(got[2], ref[2], ys, what + " lpd", mean=True)
            _close(np.array([got[3]]), np.array([ref[3]]), ys, what + " lpd_joint", mean=True)
        if m == 1:
            assert abs(ref[3] - ref[2][0]) <= FRAC * np.max(bound(ref[2], ys, mean=True))
        if m > 1:      # the mean treatment for everybody moves every output by 1e6 bounds
            alt = nv.score(c, s, Xn, Un, m, np.full(m, np.mean(Tt)), Yt, "structured")
            got = nv.score(c, s, Xn, Un, m, Tt, Yt, "structured")
            for k, (what, mean) in enumerate((("mean", True), ("var", False), ("lpd", True), ("lpd_joint", True))):
                d, b = np.max(np.abs(alt[k] - got[k])), np.max(bound(np.atleast_1d(got[k]), ys, mean))
                print(f"s={s} {what} moves by {d:.3e} = {d / b:.3e} bounds")
                assert d >= 1e6 * b, what


def test_the_chain_rule_holds_in_the_restatement():
    """log N(Y_pooled) - log N(Y_train) = lpd_joint: the device test's bound is 1e-9 (|logpdf_pooled| + |logpdf_train|), the
    restatement sits within 1e-3 of it"""
    c, Xn, Un, Tt, Yt = nv.score_case(*nv.CHAIN)
    cp = nv.pooled(c, Xn, Un, Tt, Yt)
    for s in range(c["S"]):
        lp = [orc.y_logpdf(None if k["uyLS"] is None else k["uyLS"][:, s], None if k["xyLS"] is None else k["xyLS"][:, s],
                           float(k["tyLS"][s]), float(k["yScale"][s]), float(k["yNoise"][s]),
                           None if k["U"] is None else k["U"][:, :, s], k["X"], k["T"], k["Y"]) for k in (cp, c)]
        joint = nv.score(c, s, Xn, Un, nv.CHAIN[3], Tt, Yt)[3]
        b = 1e-9 * (abs(lp[0]) + abs(lp[1]))
        print(f"s={s} pooled {lp[0]:.6f} train {lp[1]:.6f} joint {joint:.6f} err / bound {abs(lp[0] - lp[1] - joint) / b:.3e}")
        assert abs(lp[0] - lp[1] - joint) <= FRAC * b


def test_a_constant_dose_is_the_scalar_restatement():
    import new_individuals_restatement as nr
    c, Xn, Un, _, _ = nv.grid_case("UX", False, 24, 5, 5, "contrast")
    levels = nr.pairs("contrast", 2)
    A_ = np.tile(np.array([[a for a, _ in levels]]), (5, 1))
    B_ = np.tile(np.array([[b for _, b in levels]]), (5, 1))
    got, ref = nv.literal(c, 0, Xn, Un, 5, "contrast", A_, B_), nr.literal(c, 0, Xn, Un, 5, "contrast", levels)
    for g, r in zip(got, ref):
        assert np.allclose(g, r, rtol=1e-12, atol=1e-14)


def test_a_row_whose_dose_equals_its_baseline_is_zero():
    c, Xn, Un, A_, B_ = nv.grid_case("UX", False, 24, 5, 5, "contrast")
    mean, var, cov = nv.structured(c, 0, Xn, Un, 5, "contrast", A_, B_)
    off = cov[:, 1, [0, 2, 3, 4]]
    assert not mean[1].any() and np.array_equal(var[1], np.full(5, nv.PN)) and not off.any() and mean[0].all()


# ---- the front end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gp_front():
    import causalgpslc_jl_amd as gp_
    return gp_


D2 = np.array([[0.6, 0.1, -0.2], [0.3, 0.2, 0.9]])      # (L, m) = (2, 3)
REFUSALS = [
    (dict(doTs=D2, Tnew=[0.1, 0.2, 0.3], baseline=0.1), "Tnew= cannot be combined with baseline="),
    (dict(doTs=[0.6], Tnew=[0.1, 0.2, 0.3], slope=True), "Tnew= cannot be combined with slope=True"),
    (dict(doTs=D2, slope=True), "slope=True needs scalar levels"),
    (dict(doTs=np.zeros((2, 2, 3))), "needs scalar levels or an (L, m) array"),
    (dict(doTs=np.zeros((2, 4))), "(L, m) array of per-individual levels with m = 3"),
    (dict(doTs=[0.6], Tnew=[0.1, 0.2]), "Tnew must be a vector of m = 3"),
    (dict(doTs=[0.6], Tnew=[0.1, np.nan, 0.2]), "Tnew has a non-finite entry"),
    (dict(doTs=D2, baseline=np.zeros((3, 2))), "baseline must be a scalar, one value per level (L = 2) or an (L, m) array"),
    (dict(doTs=D2, baseline=[0.1, 0.2, 0.3]), "baseline must be a scalar or one value per level"),
    (dict(doTs=np.where(D2 > 0.8, np.inf, D2)), "doTs has a non-finite entry"),
]


@pytest.mark.parametrize("kw,message", REFUSALS)
def test_refusals_come_before_any_library_call(gp_front, kw, message):
    kw = dict(kw)
    doTs = kw.pop("doTs")
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.predictNew(_obj(gp_front), doTs, Xnew=XN, like=[0, 1, 2], **kw)
        assert lib.calls == []
    assert message in str(ei.value)


def test_average_new_keeps_scalar_levels(gp_front):
    with recording(gp_front) as lib:
        with pytest.raises(ValueError) as ei:
            gp_front.averageNew(_obj(gp_front), D2, Xnew=XN, like=[0, 1, 2])
        assert lib.calls == []
    assert "needs scalar levels" in str(ei.value) and "(L, m)" not in str(ei.value)


def _vec_calls(lib):
    return [c[1] for c in lib.calls if c[0] == "gpslc_predict_new_vec"]


def test_two_dimensional_levels_reach_the_vector_entry_point(gp_front):
    g = _obj(gp_front)
    with recording(gp_front) as lib:
        mean, var, cov = gp_front.predictNew(g, D2, Xnew=XN, like=[3, 0, 7], want_cov=True)
        gp_front.predictNew(g, D2, Xnew=XN, like=[3, 0, 7], baseline=0.1)
        gp_front.predictNew(g, D2, Xnew=XN, like=[3, 0, 7], baseline=[0.1, 0.2])
        gp_front.predictNew(g, D2, Xnew=XN, like=[3, 0, 7], baseline=D2[::-1])
    assert [c[0] for c in lib.calls][:3] == ["gpslc_create", "gpslc_set_data", "gpslc_predict_new_vec"]
    assert not [c for c in lib.calls if c[0] == "gpslc_predict_new"]
    e = _vec_calls(lib)
    assert (e[0]["S"], e[0]["m"], e[0]["form"], e[0]["L"], e[0]["pred_noise"], e[0]["doT_base"]) == (2, 3, 0, 2, 1e-10, None)
    assert e[0]["doT"] == _array(np.asfortranarray(D2.T)) and e[0]["doT"].startswith("f8[3, 2]/[8, 24]")
    assert e[0]["Unew"] == _array(np.asfortranarray(CASE["U"][[3, 0, 7]]))
    assert e[0]["mean"] == e[0]["var"] == "f8[3, 2, 2]/[8, 24, 48]" and e[0]["cov"] == "f8[3, 3, 2, 2]/[8, 24, 72, 144]"
    assert mean.shape == var.shape == (3, 2, 2) and cov.shape == (2, 2, 3, 3)
    assert [x["form"] for x in e[1:]] == [1, 1, 1]
    assert e[1]["doT_base"] == _array(np.asfortranarray(np.full((3, 2), 0.1)))
    assert e[2]["doT_base"] == _array(np.asfortranarray(np.tile([[0.1, 0.2]], (3, 1))))
    assert e[3]["doT_base"] == _array(np.asfortranarray(D2[::-1].T))


def test_tnew_is_the_baseline_of_every_level(gp_front):
    g, Tn = _obj(gp_front), np.array([0.5, -0.5, 0.25])
    with recording(gp_front) as lib:
        gp_front.predictNew(g, [0.6, 0.2], Xnew=XN, Unew=UN, Tnew=Tn)            # scalar levels, per-individual baseline
        gp_front.predictNew(g, D2, Xnew=XN, Unew=UN, Tnew=Tn, want_var=False)
    e = _vec_calls(lib)
    assert len(e) == 2 and [x["form"] for x in e] == [1, 1] and [x["L"] for x in e] == [2, 2]
    assert e[0]["doT"] == _array(np.asfortranarray(np.tile([[0.6, 0.2]], (3, 1))))
    assert e[0]["doT_base"] == e[1]["doT_base"] == _array(np.asfortranarray(np.tile(Tn[:, None], (1, 2))))
    assert e[1]["doT"] == _array(np.asfortranarray(D2.T)) and e[1]["var"] is None and e[1]["cov"] is None


def test_the_test_set_call_and_its_summary(gp_front):
    g = _obj(gp_front)
    Tt, Yt = np.array([0.5, -0.5, 0.25]), np.array([1.0, 0.0, -1.0])
    with recording(gp_front) as lib:
        out = gp_front.testPredictive(g, XN, Tt, Yt, like=[3, 0, 7])
        summ = gp_front.testSummary(g, XN, Tt, Yt, like=[3, 0, 7], test=out)
        for kw, message in ((dict(Ttest=Tt[:2], Ytest=Yt), "Ttest must be a vector of m = 3"), (dict(Ttest=Tt), "needs Ttest= and Ytest="),
                            (dict(Ttest=Tt, Ytest=[1.0, np.inf, 0.0]), "Ytest has a non-finite entry")):
            with pytest.raises(ValueError) as ei:
                gp_front.testPredictive(g, XN, like=[3, 0, 7], **kw)
            assert message in str(ei.value)
        with pytest.raises(ValueError) as ei:
            gp_front.testPredictive(g, None, Tt, Yt, like=[3, 0, 7])
        assert "Xtest= is required" in str(ei.value)
    assert [c[0] for c in lib.calls] == ["gpslc_create", "gpslc_set_data", "gpslc_y_test"]
    e = lib.calls[2][1]
    assert (e["S"], e["m"]) == (2, 3) and e["Xtest"] == _array(np.asfortranarray(XN))
    assert e["Utest"] == _array(np.asfortranarray(CASE["U"][[3, 0, 7]])) and e["Ttest"] == _array(Tt) and e["Ytest"] == _array(Yt)
    assert e["mean"] == e["var"] == e["lpd"] == "f8[3, 2]/[8, 24]" and e["lpd_joint"] == "f8[2]/[8]"
    mean, var, lpd, joint = out
    assert mean.shape == var.shape == lpd.shape == (3, 2) and joint.shape == (2,)
    assert set(summ) == {"elpd", "pointwise", "zscore", "pit", "joint", "rmse"}
    assert np.array_equal(summ["elpd"], lpd.sum(axis=0)) and summ["joint"] is joint and summ["pointwise"].shape == (3,)
    assert np.allclose(summ["rmse"], np.sqrt(np.mean((Yt[:, None] - mean) ** 2, axis=0)))
    assert np.array_equal(summ["zscore"], (Yt[:, None] - mean) / np.sqrt(var))


def test_the_symbols_are_declared_and_bound(gp_front):
    from causalgpslc_jl_amd import _lib
    for sym in ("gpslc_predict_new_vec", "gpslc_y_test"):
        assert sym in _lib.header_symbols() and sym in _lib.SIGNATURES
