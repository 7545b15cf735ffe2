"""Predictions for new individuals on the GPU (gpslc_predict_new, `predictNew`) against the dense restatement in
tests/new_individuals_restatement.py (its literal side), against the library's own ITEDistributions where the new individuals
copy training rows, and bit for bit where the call's own guarantees say so.

Bounds: test_gpu_contrast._check's, imported and not restated — mean 1e-6 max|ref| + 1e-12 then 1e-9 max|ref| + 1e-13 (its
MeanITE check), var 1e-6 |ref| + 1e-9 yScale then 1e-9 |ref| + 1e-12 yScale per element (its varSATE check, the (individual,
level) pairs folded into its level axis), cov the same with |ref| the block's largest entry (one scalar per block: the largest
entry against itself plus the block's largest error).  No bound of this file is its own.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import new_individuals_restatement as nr
from test_gpu_contrast import _check

pytestmark = pytest.mark.gpu
PN = nr.PN


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check_new(exp, mean, var, cov, case, samples=None):
    """mean, var (m, S, L), cov (S, L, m, m) or None against exp's, through test_gpu_contrast._check"""
    m, S, L = mean.shape
    zeros = lambda *shape: np.zeros(shape)
    print("mean")
    _check(dict(meanSATE=zeros(S, L), varSATE=zeros(S, L), meanITE=exp["mean"]), zeros(S, L), zeros(S, L), mean, case, samples)
    if var is not None:
        print("var, level axis = (individual, level)")
        fold = lambda a: np.transpose(a, (1, 0, 2)).reshape(S, m * L)
        _check(dict(meanSATE=zeros(S, m * L), varSATE=fold(exp["var"]), meanITE=zeros(1, S, m * L)), zeros(S, m * L), fold(var),
               zeros(1, S, m * L), case, samples)
    if cov is not None:
        print("cov, one scalar per block: its largest entry, moved by its largest error")
        top = np.max(np.abs(exp["cov"]), axis=(2, 3))
        err = np.max(np.abs(cov - exp["cov"]), axis=(2, 3))
        _check(dict(meanSATE=zeros(S, L), varSATE=top, meanITE=zeros(1, S, L)), zeros(S, L), top + err, zeros(1, S, L), case, samples)


@functools.lru_cache(maxsize=None)
def _case(n, shape, binary_t=False, S=2, seed=0):
    return cases.make_case(n, shape, binary_t, S=S, seed=90 + seed + n)


@functools.lru_cache(maxsize=None)
def _object(gp, n, shape, binary_t=False, S=2, seed=0):
    return cases.gpslc_object(gp, _case(n, shape, binary_t, S, seed))


def _levels(form, L):
    lv = nr.pairs(form, L)
    doT = np.array([a for a, _ in lv])
    return lv, doT, (np.array([b for _, b in lv]) if form == "contrast" else None)


def _call(g, m, Xn, Un, form, doT, base, want=("mean", "var", "cov"), pred_noise=PN):
    return g.ctx().predict_new(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, doT,
                               base, pred_noise, want=want)


def _cov_slnn(cov):
    return None if cov is None else np.transpose(cov, (2, 3, 0, 1))


# ---- 1. against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("L", [1, 5, 65])
@pytest.mark.parametrize("m", [1, 5, 128, 129, 300])
@pytest.mark.parametrize("n", [24, 129, 200])
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_against_restatement(gp, shape, n, m, L, form):
    """a single new individual, a second row tile with one live row, more row tiles than the factor has (m = 300), the second
    64-column pass of the mean (L = 65) and, on two tiles with S = 2, 130 pairs for sub-batches of 128; shape T: no features,
    both pointers NULL.  The covariance where m <= 129 and L <= 5."""
    c, g = _case(n, shape), _object(gp, n, shape)
    Xn, Un = nr.new_individuals(c, m, seed=m + L)
    lv, doT, base = _levels(form, L)
    want_cov = m <= 129 and L <= 5
    st, mean, var, cov = _call(g, m, Xn, Un, form, doT, base, want=("mean", "var") + (("cov",) if want_cov else ()))
    assert st == 0 and (Xn is None) == (shape in "UT") and (Un is None) == (shape in "XT")
    assert mean.shape == var.shape == (m, 2, L) and (cov is None or cov.shape == (m, m, 2, L))
    _check_new(nr.expected(c, Xn, Un, m, form, lv, want_cov=want_cov), mean, var, _cov_slnn(cov), c)


@pytest.mark.parametrize("form", nr.FORMS)
def test_binary_treatment_through_the_c_entry_point(gp, form):
    n, S, m, L = 129, 2, 5, 3
    c = cases.make_case(n, "UX", True, S=S, seed=92)
    g = cases.gpslc_object(gp, c)
    Xn, Un = nr.new_individuals(c, m, seed=3)
    lv = [(0.0, 1.0), (1.0, 0.0), (0.5, 0.2)] if form == "contrast" else [(0.0, None), (1.0, None), (0.5, None)]
    doT = np.array([a for a, _ in lv])
    base = np.array([b for _, b in lv]) if form == "contrast" else None
    mean, var = np.empty((m, S, L), order="F"), np.empty((m, S, L), order="F")
    cov = np.empty((m, m, S, L), order="F")
    ctx = g.ctx()
    st = ctx.lib.gpslc_predict_new(ctx.h, S, *g._params(), m, _p(Xn), _p(Un), gp.api.NEW_FORMS[form], L, _p(doT), _p(base), PN,
                                   _p(mean), _p(var), _p(cov))
    assert st == 0
    _check_new(nr.expected(c, Xn, Un, m, form, lv), mean, var, _cov_slnn(cov), c)


# ---- 2. identity with the existing path -----------------------------------------------------------------------------------
IDX = [0, 5, 127, 128, 199, 64]          # both tiles of n = 200


@pytest.mark.parametrize("kw", [dict(), dict(baseline=-0.3), dict(slope=True)], ids=["outcome", "contrast", "slope"])
@pytest.mark.parametrize("shape", ["UX", "X"])
def test_copies_of_training_rows_reproduce_ite_distributions(gp, shape, kw):
    c, g = _case(200, shape), _object(gp, 200, shape)
    a = 0.6
    M, Cv = gp.ITEDistributions(g, a, outcome=not kw, **kw)
    mean, var, cov = gp.predictNew(g, a, Xnew=c["X"][IDX], like=IDX if shape == "UX" else None, want_cov=True, **kw)
    exp = dict(mean=M[:, IDX].T[:, :, None], var=np.stack([np.diag(Cv[s])[IDX] for s in range(2)], axis=1)[:, :, None],
               cov=np.stack([Cv[s][np.ix_(IDX, IDX)] for s in range(2)])[:, None])
    _check_new(exp, mean, var, cov, c)
    # two copies of one training individual in one call: the same bits twice (their covariance carries no pred_noise: they are
    # two individuals)
    twin = [5, 199, 5]
    mean2, var2 = gp.predictNew(g, a, Xnew=c["X"][twin], like=twin if shape == "UX" else None, **kw)
    assert np.array_equal(mean2[0], mean2[2]) and np.array_equal(var2[0], var2[2])
    assert np.array_equal(mean2[:2], mean[[1, 4]]) and np.array_equal(var2[:2], var[[1, 4]])


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_a_contrast_of_a_level_with_itself_is_exactly_zero(gp, shape):
    c, g = _case(200, shape), _object(gp, 200, shape)
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=4)
    A = np.array([0.37, 0.6, 0.37, -1.2, 0.37, 0.37])       # L = 6: two real contrasts among the equal pairs
    B = np.array([0.37, -0.3, 0.37, 0.5, 0.37, 0.37])
    st, mean, var, cov = _call(g, m, Xn, Un, "contrast", A, B)
    assert st == 0
    off = ~np.eye(m, dtype=bool)
    for l in range(6):
        same = A[l] == B[l]
        assert (not mean[:, :, l].any()) == same
        assert np.array_equal(var[:, :, l], np.full((m, 2), PN)) == same
        assert (not cov[:, :, :, l][off].any()) == same


# ---- 3. bits --------------------------------------------------------------------------------------------------------------
def test_permutations_and_subsets_keep_every_individuals_bits(gp):
    c, g = _case(200, "UX"), _object(gp, 200, "UX")
    m = 140
    Xn, Un = nr.new_individuals(c, m, seed=5)
    _, doT, base = _levels("contrast", 5)
    st, mean, var, cov = _call(g, m, Xn, Un, "contrast", doT, base)
    assert st == 0
    perm = np.random.default_rng(6).permutation(m)
    for idx in (perm, perm[:3], np.array([139]), np.arange(128)):
        k = len(idx)
        st, mean2, var2, cov2 = _call(g, k, np.asfortranarray(Xn[idx]), np.asfortranarray(Un[idx]), "contrast", doT, base)
        assert st == 0
        assert np.array_equal(mean2, mean[idx]) and np.array_equal(var2, var[idx])
        for i in range(k):
            assert np.array_equal(cov2[i, i], var2[i])
    assert np.array_equal(cov, np.transpose(cov, (1, 0, 2, 3)))
    assert np.array_equal(np.einsum("iisl->isl", cov), var)


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    c = _case(200, "UX", S=3)
    m = 129
    Xn, Un = nr.new_individuals(c, m, seed=7)
    lv, doT, base = _levels("slope", 3)
    ref = _call(cases.gpslc_object(gp, c), m, Xn, Un, "slope", doT, base)
    assert ref[0] == 0
    for tuning in (dict(max_batch=1), dict(n_streams=1), dict(n_streams=3), dict(max_batch=1, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            got = _call(g, m, Xn, Un, "slope", doT, base)
            assert got[0] == 0
            for x, y in zip(ref[1:], got[1:]):
                assert np.array_equal(x, y), (tuning, rep)
    _check_new(nr.expected(c, Xn, Un, m, "slope", lv, samples=(2,)), ref[1], ref[2], _cov_slnn(ref[3]), c, samples=(2,))


def test_schedules_give_the_same_bits(gp):
    """five tiles: the factor and alpha from the persistent launch against the per-column schedule's"""
    from test_gpu_outcome import _forced_schedules
    c = _case(520, "UX")
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=8)
    lv, doT, base = _levels("outcome", 2)
    out = _forced_schedules(gp, c, lambda g: _call(g, m, Xn, Un, "outcome", doT, base))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert out[0][0] == 0
    _check_new(nr.expected(c, Xn, Un, m, "outcome", lv, samples=(1,)), out[0][1], out[0][2], _cov_slnn(out[0][3]), c, samples=(1,))


def test_each_output_alone(gp):
    c, g = _case(129, "UX"), _object(gp, 129, "UX")
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=9)
    _, doT, base = _levels("contrast", 2)
    full = _call(g, m, Xn, Un, "contrast", doT, base)
    assert full[0] == 0
    for k, name in enumerate(("mean", "var", "cov"), start=1):
        one = _call(g, m, Xn, Un, "contrast", doT, base, want=(name,))
        assert one[0] == 0
        for j in range(1, 4):
            assert (one[j] is None) == (j != k)
        assert np.array_equal(one[k], full[k]), name


# ---- 4. breakdown and argument errors ---------------------------------------------------------------------------------------
def test_breakdown_gives_nan_for_that_sample_only(gp):
    """test_gpu_loo's construction — yNoise = 0 and a duplicated individual in a model without U and X: sample 0's matrix is
    singular (pivot 2 is exactly 0); an ordinary error return"""
    c = dict(cases.make_case(200, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    m = 3
    lv, doT, base = _levels("outcome", 2)
    st, mean, var, cov = _call(g, m, None, None, "outcome", doT, base)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for a in (mean, var):
        assert np.isnan(a[:, 0]).all()
    assert np.isnan(cov[:, :, 0]).all()
    _check_new(nr.expected(c, None, None, m, "outcome", lv, samples=(1,)), mean, var, _cov_slnn(cov), c, samples=(1,))
    with pytest.raises(gp.PosDefException) as ei:
        gp.predictNew(g, doT)
    assert ei.value.info == 2
    # the context keeps working
    c["yNoise"] = np.array([c["yNoise"][1], c["yNoise"][1]])
    g2 = cases.gpslc_object(gp, c)
    g2._ctx = g.ctx()
    mean2, var2 = gp.predictNew(g2, doT)
    assert mean2.shape == (1, 2, 2) and np.isfinite(mean2).all() and (var2 > 0).all()


def test_argument_errors(gp):
    c = _case(24, "UX")
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    m = 3
    Xn, Un = nr.new_individuals(c, m)
    doT, base = np.array([0.6, 0.2]), np.array([0.1, 0.1])

    def call(m=m, Xn=Xn, Un=Un, form="outcome", doT=doT, base=None, want=("mean", "var"), ctx=ctx):
        return ctx.predict_new(2, g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, doT, base, PN, want=want)[0]

    def message():
        return ctx.lib.gpslc_last_error(ctx.h).decode()

    assert call(m=0) == -9 and "m < 1" in message()
    assert call(doT=None) == -13 and "L < 1" in message()                       # L = 0
    assert call(form=3) == -12 and "factual" in message()                       # unknown form: the text says why none is ordinary
    assert call(form="contrast") == -15 and "doT_base is NULL" in message()
    assert call(base=base) == -15 and "no contrast" in message()
    assert call(form="slope", base=base) == -15
    assert call(Xn=None) == -10 and "Xnew is NULL" in message()
    assert call(Un=None) == -11 and "Unew is NULL" in message()
    bad = Xn.copy(order="F")
    bad[1, 1] = np.nan
    assert call(Xn=bad) == -10 and "non-finite" in message()
    bad = Un.copy(order="F")
    bad[2, 0, 1] = np.inf
    assert call(Un=bad) == -11 and "non-finite" in message()
    assert call(doT=np.array([0.6, np.nan])) == -14 and "non-finite" in message()
    assert call(want=()) == -17 and "all NULL" in message()
    assert call() == 0                                                          # the context stays usable
    # a model without features refuses what it has no use for
    gT = cases.gpslc_object(gp, _case(24, "T"))
    cT = gT.ctx()
    args = (2, None, None, None, gT.tyLS, gT.yScale, gT.yNoise)
    assert cT.predict_new(*args, m, Xn, None, "outcome", doT, None, PN)[0] == -10
    assert cT.predict_new(*args, m, None, Un, "outcome", doT, None, PN)[0] == -11
    assert cT.predict_new(*args, m, None, None, "outcome", doT, None, PN)[0] == 0
    # an fp32 context
    g32 = cases.gpslc_object(gp, c, fp32_kernel=True)
    assert call(ctx=g32.ctx()) == -1007
    assert "fp64" in g32.ctx().lib.gpslc_last_error(g32.ctx().h).decode()
    assert np.isfinite(gp.predict(g32, doT)[0]).all()                           # and goes on serving what it supports
    fresh = gp.Context(24, 3, 2)
    assert call(ctx=fresh) == -1002                                             # GPSLC_ERR_NODATA
    assert call() == 0
