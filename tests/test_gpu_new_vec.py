"""New individuals at per-individual levels and the score of a held-out test set on the GPU (gpslc_predict_new_vec, gpslc_y_test,
`predictNew` with 2-D levels / `Tnew=`, `testPredictive`) against the dense restatement in
tests/new_vec_restatement.py (its literal side; tests/test_new_vec.py holds that side to 1e-3 of the bounds used here on these
very cases), against three existing paths of the library (the scalar call, the vector levels of the training rows, the ordinary
ITE distributions; the pooled log density), and bit for bit where the calls' own guarantees say so.

Bounds: test_gpu_contrast._check's two stages through test_gpu_new_individuals._check_new, imported and not restated; log densities
take the bound of a mean.  The chain rule's bound is 1e-9 (|logpdf_pooled| + |logpdf_train|)."""
import numpy as np
import pytest

import cases
import new_individuals_restatement as nr
import new_vec_restatement as nv
import test_gpu_new_individuals as tn

pytestmark = pytest.mark.gpu
PN = nv.PN
_check_new, _cov_slnn = tn._check_new, tn._cov_slnn


def _call(g, m, Xn, Un, form, A_, B_, want=("mean", "var", "cov"), pred_noise=PN):
    return g.ctx().predict_new_vec(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, A_,
                                   B_, pred_noise, want=want)


def _score(g, m, Xn, Un, Tt, Yt, **kw):
    return g.ctx().y_test(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, Tt, Yt, **kw)


# ---- 1, 4, 5. against the restatement; rows with a == b; symmetry and the diagonal ----------------------------------------------
@pytest.mark.parametrize("shape,bt,n,m,L,form,with_cov", nv.GRID)
def test_against_restatement(gp, shape, bt, n, m, L, form, with_cov):
    c, Xn, Un, A_, B_ = nv.grid_case(shape, bt, n, m, L, form)
    g = cases.gpslc_object(gp, c)
    st, mean, var, cov = _call(g, m, Xn, Un, form, A_, B_, want=("mean", "var") + (("cov",) if with_cov else ()))
    assert st == 0 and mean.shape == var.shape == (m, 2, L) and (cov is None or cov.shape == (m, m, 2, L))
    _check_new(nv.expected(c, Xn, Un, m, form, A_, B_, want_cov=with_cov), mean, var, _cov_slnn(cov), c)
    if with_cov:
        assert np.array_equal(cov, np.transpose(cov, (1, 0, 2, 3)))
        assert np.array_equal(np.einsum("iisl->isl", cov), var)
    if form == "contrast" and m > 1:      # row 1 has b == a at every level: exact zeros, and the other rows have none
        assert not mean[1].any() and np.array_equal(var[1], np.full((2, L), PN))
        assert mean[0].all() and (var[0] != PN).all()
        if with_cov:
            others = [i for i in range(m) if i != 1]
            assert not cov[1, others].any() and not cov[others, 1].any()


# ---- 2. constant doses are the scalar call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", nv.FORMS)
def test_constant_doses_agree_with_the_scalar_call(gp, form):
    n, m, L = 129, 130, 5
    c = cases.make_case(n, "UX", False, S=2, seed=301)
    g = cases.gpslc_object(gp, c)
    Xn, Un = nr.new_individuals(c, m, seed=12)
    lv = nr.pairs(form, L)
    doT = np.array([a for a, _ in lv])
    base = np.array([b for _, b in lv]) if form == "contrast" else None
    st, mean0, var0, cov0 = tn._call(g, m, Xn, Un, form, doT, base)
    assert st == 0
    tile = lambda v: None if v is None else np.asfortranarray(np.tile(v[None, :], (m, 1)))
    st, mean, var, cov = _call(g, m, Xn, Un, form, tile(doT), tile(base))
    assert st == 0
    _check_new(dict(mean=mean0, var=var0, cov=_cov_slnn(cov0)), mean, var, _cov_slnn(cov), c)


# ---- 3. copies of training rows -----------------------------------------------------------------------------------------------
ROWS = [0, 5, 127, 128]


def test_copies_of_training_rows_at_their_own_doses(gp):
    n, L = 129, 3
    c = cases.make_case(n, "UX", False, S=2, seed=302)
    g = cases.gpslc_object(gp, c)
    D = np.random.default_rng(3).uniform(-1.5, 1.5, size=(L, n))
    _, _, mi = gp.predict(g, D, want_mean_ite=True, outcome=True)                 # (n, S, L): f_i(d_i) of the training rows
    mean, _ = gp.predictNew(g, D[:, ROWS], Xnew=c["X"][ROWS], like=ROWS)
    _check_new(dict(mean=mi[ROWS]), mean, None, None, c)


def test_tnew_gives_the_ordinary_effect_of_copied_rows(gp):
    n, a = 129, 0.6
    c = cases.make_case(n, "UX", False, S=2, seed=303)
    g = cases.gpslc_object(gp, c)
    M, Cv = gp.ITEDistributions(g, a)                                               # the reference's f(a) - f(T_i)
    Tn = c["T"][ROWS]
    mean, var = gp.predictNew(g, a, Xnew=c["X"][ROWS], like=ROWS, Tnew=Tn)
    exp = dict(mean=M[:, ROWS].T[:, :, None], var=np.stack([np.diag(Cv[s])[ROWS] for s in range(2)], axis=1)[:, :, None])
    _check_new(exp, mean, var, None, c)
    # per-individual doses with one at its own treatment: exactly zero there, and nowhere else
    D = np.array([[a, Tn[1], a, -0.4]])
    mean, var = gp.predictNew(g, D, Xnew=c["X"][ROWS], like=ROWS, Tnew=Tn)
    assert not mean[1].any() and np.array_equal(var[1], np.full((2, 1), PN)) and mean[[0, 2, 3]].all()


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------
def test_permutations_and_subsets_keep_every_individuals_bits(gp):
    n, m, L = 200, 140, 5
    c = cases.make_case(n, "UX", False, S=2, seed=304)
    g = cases.gpslc_object(gp, c)
    Xn, Un = nr.new_individuals(c, m, seed=5)
    A_, B_ = nv.doses(m, L, "contrast", seed=6, equal_rows=(3,))
    st, mean, var, cov = _call(g, m, Xn, Un, "contrast", A_, B_)
    assert st == 0
    perm = np.random.default_rng(6).permutation(m)
    take = lambda V, idx: np.asfortranarray(V[idx])
    for idx in (perm, perm[:3], np.array([139]), np.arange(128)):
        st, mean2, var2, cov2 = _call(g, len(idx), take(Xn, idx), take(Un, idx), "contrast", take(A_, idx), take(B_, idx))
        assert st == 0
        assert np.array_equal(mean2, mean[idx]) and np.array_equal(var2, var[idx])
        assert np.array_equal(np.einsum("iisl->isl", cov2), var2)


def test_chunking_and_streams_give_the_same_bits(gp):
    n, m, L = 200, 129, 3
    c = cases.make_case(n, "UX", False, S=3, seed=305)
    Xn, Un = nr.new_individuals(c, m, seed=7)
    A_, B_ = nv.doses(m, L, "contrast", seed=8)
    Tt, Yt = nv.held_out(c, m, seed=9)
    ref = _call(cases.gpslc_object(gp, c), m, Xn, Un, "contrast", A_, B_) + _score(cases.gpslc_object(gp, c), m, Xn, Un, Tt, Yt)
    assert ref[0] == 0 and ref[4] == 0
    for tuning in (dict(max_batch=1), dict(n_streams=1), dict(n_streams=3), dict(max_batch=1, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        got = _call(g, m, Xn, Un, "contrast", A_, B_) + _score(g, m, Xn, Un, Tt, Yt)
        for x, y in zip(ref, got):
            assert np.array_equal(x, y), tuning


def test_schedules_give_the_same_bits(gp):
    from test_gpu_outcome import _forced_schedules
    n, m, L = 200, 130, 2
    c = cases.make_case(n, "UX", False, S=2, seed=306)
    Xn, Un = nr.new_individuals(c, m, seed=8)
    A_, _ = nv.doses(m, L, "outcome", seed=9)
    Tt, Yt = nv.held_out(c, m, seed=10)
    out = _forced_schedules(gp, c, lambda g: _call(g, m, Xn, Un, "outcome", A_, None) + _score(g, m, Xn, Un, Tt, Yt))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert out[0][0] == 0 and out[0][4] == 0


# ---- 7. the test-set score ------------------------------------------------------------------------------------------------------
def _joint_close(got, ref, what):
    err, b = np.abs(got - ref), 1e-9 * np.abs(ref) + 1e-13
    print(what, "err", err, "bound", b)
    assert np.all(err <= b), what


@pytest.mark.parametrize("shape,bt,n,m", nv.SCORE_GRID)
def test_score_against_restatement(gp, shape, bt, n, m):
    c, Xn, Un, Tt, Yt = nv.score_case(shape, bt, n, m)
    g = cases.gpslc_object(gp, c)
    mean, var, lpd, joint = gp.testPredictive(g, Xn, Tt, Yt, Utest=Un)
    assert mean.shape == var.shape == lpd.shape == (m, 2) and joint.shape == (2,)
    exp = nv.expected_score(c, Xn, Un, m, Tt, Yt)
    _check_new(dict(mean=exp["mean"][:, :, None], var=exp["var"][:, :, None]), mean[:, :, None], var[:, :, None], None, c)
    _check_new(dict(mean=exp["lpd"][:, :, None]), lpd[:, :, None], None, None, c)
    _joint_close(joint, exp["joint"], "lpd_joint against the restatement")
    host = -0.5 * nv.LOG2PI - 0.5 * np.log(var) - 0.5 * (Yt[:, None] - mean) ** 2 / var
    _check_new(dict(mean=host[:, :, None]), lpd[:, :, None], None, None, c)
    if m == 1:
        _joint_close(joint, lpd[0], "lpd_joint against lpd at m = 1")
    # each output alone: the same bits
    for k, name in enumerate(("mean", "var", "lpd", "joint")):
        one = _score(g, m, Xn, Un, Tt, Yt, want=(name,))
        assert one[0] == 0 and [o is None for o in one[1:]] == [j != k for j in range(4)]
        assert np.array_equal(one[1 + k], (mean, var, lpd, joint)[k]), name


# ---- 8. the chain rule through gpslc_y_logpdf -------------------------------------------------------------------------------------
def test_the_joint_density_is_the_difference_of_two_log_densities(gp):
    c, Xn, Un, Tt, Yt = nv.score_case(*nv.CHAIN)
    g = cases.gpslc_object(gp, c)
    lp_train = gp.yLogpdf(g)
    lp_pooled = gp.yLogpdf(cases.gpslc_object(gp, nv.pooled(c, Xn, Un, Tt, Yt)))
    joint = gp.testPredictive(g, Xn, Tt, Yt, Utest=Un)[3]
    err, b = np.abs((lp_pooled - lp_train) - joint), 1e-9 * (np.abs(lp_pooled) + np.abs(lp_train))
    print("pooled", lp_pooled, "train", lp_train, "joint", joint, "err", err, "bound", b)
    assert np.all(err <= b)


# ---- 9. breakdown and refusals ------------------------------------------------------------------------------------------------
def test_breakdown_gives_nan_for_that_sample_only(gp):
    """test_gpu_new_individuals' construction: sample 0's A is singular (pivot 2 is exactly 0)"""
    c = dict(cases.make_case(200, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    m = 3
    A_, _ = nv.doses(m, 2, "outcome", seed=1)
    st, mean, var, cov = _call(g, m, None, None, "outcome", A_, None)
    assert st == 2 and list(g.ctx().last_info(2)) == [2, 0]
    assert np.isnan(mean[:, 0]).all() and np.isnan(var[:, 0]).all() and np.isnan(cov[:, :, 0]).all()
    _check_new(nv.expected(c, None, None, m, "outcome", A_, None, samples=(1,)), mean, var, _cov_slnn(cov), c, samples=(1,))
    Tt, Yt = nv.held_out(c, m, seed=2)
    st, mean, var, lpd, joint = _score(g, m, None, None, Tt, Yt)
    assert st == 2 and list(g.ctx().last_info(2)) == [2, 0]
    assert all(np.isnan(a[:, 0]).all() for a in (mean, var, lpd)) and np.isnan(joint[0])
    exp = nv.expected_score(c, None, None, m, Tt, Yt, samples=(1,))
    _check_new(dict(mean=exp["lpd"][:, :, None]), lpd[:, :, None], None, None, c, samples=(1,))
    _joint_close(joint[1], exp["joint"][1], "lpd_joint of the intact sample")
    with pytest.raises(gp.PosDefException) as ei:
        gp.testPredictive(g, None, Tt, Yt)
    assert ei.value.info == 2


def test_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=307)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    m = 3
    Xn, Un = nr.new_individuals(c, m)
    A_, B_ = nv.doses(m, 2, "contrast", seed=1)
    Tt, Yt = nv.held_out(c, m, seed=2)

    def call(m=m, Xn=Xn, Un=Un, form="outcome", doT=A_, base=None, want=("mean", "var"), ctx=ctx):
        return ctx.predict_new_vec(2, g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, doT, base, PN, want=want)[0]

    def score(m=m, Xn=Xn, Un=Un, Tt=Tt, Yt=Yt, want=("mean", "var", "lpd", "joint"), ctx=ctx):
        return ctx.y_test(2, g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, Tt, Yt, want=want)[0]

    def message():
        return ctx.lib.gpslc_last_error(ctx.h).decode()

    def spoil(a, at, v=np.nan):
        a = a.copy(order="F")
        a[at] = v
        return a

    assert call(m=0) == -9 and "m < 1" in message()
    assert call(doT=None) == -13 and "L < 1" in message()
    assert call(form=3) == -12 and "factual" in message()
    assert call(form="slope") == -12 and "unsupported form" in message()          # the slope at per-individual levels is refused
    assert call(form="contrast") == -15 and "doT_base is NULL" in message()
    assert call(base=B_) == -15 and "no contrast" in message()
    assert call(Xn=None) == -10 and call(Un=None) == -11
    assert call(Xn=spoil(Xn, (1, 1))) == -10 and call(Un=spoil(Un, (2, 0, 1), np.inf)) == -11
    assert call(doT=spoil(A_, (2, 1))) == -14 and "non-finite" in message()        # the LAST entry of the m x L array is read
    assert call(form="contrast", base=spoil(B_, (2, 1))) == -15 and "non-finite" in message()
    assert call(want=()) == -17 and "all NULL" in message()
    assert call() == 0 and call(form="contrast", base=B_) == 0
    assert score(m=0) == -9
    assert score(Xn=None) == -10 and score(Un=None) == -11 and score(Un=spoil(Un, (2, 0, 1))) == -11
    assert score(Tt=None) == -12 and "Ttest is NULL" in message()
    assert score(Tt=spoil(Tt, 2)) == -12 and "non-finite" in message()
    assert score(Yt=None) == -13 and score(Yt=spoil(Yt, 2, np.inf)) == -13
    assert score(want=()) == -14 and "all NULL" in message()
    assert score() == 0
    g32 = cases.gpslc_object(gp, c, fp32_kernel=True)
    assert call(ctx=g32.ctx()) == -1007 and score(ctx=g32.ctx()) == -1007
    assert "fp64" in g32.ctx().lib.gpslc_last_error(g32.ctx().h).decode()
    fresh = gp.Context(24, 3, 2)
    assert call(ctx=fresh) == -1002 and score(ctx=fresh) == -1002
    assert call() == 0 and score() == 0
