"""Weighted averages over new individuals on the GPU (gpslc_predict_new_weighted, `averageNew`) against the dense
restatement in tests/new_average_restatement.py (its literal side), against the library's own `predictNew`, `predict(weights=)` and
`effectCurve`, and bit for bit where the call's own guarantees say so.

Bounds (tests/test_gpu_group_weights.py's, with ||w||_1 over the m weights of a column; new_average_restatement.check): required
|mean - ref| <= 1e-6 |ref| + 1e-12 ||w||_1 and |var - ref| <= 1e-6 |ref| + 1e-9 yScale ||w||_1^2, tight 1e-9 / 1e-13 and 1e-9 /
1e-12; a covariance entry off the diagonal takes the variance bounds with its own |ref|.  Every comparison asserts both."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import new_average_restatement as na
import new_individuals_restatement as nr
import new_individuals_widths as nw

pytestmark = pytest.mark.gpu
PN = nr.PN
WORST = {}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _case(n, shape, binary_t=False, S=2, seed=0):
    return cases.make_case(n, shape, binary_t, S=S, seed=120 + seed + n)


@functools.lru_cache(maxsize=None)
def _object(gp, n, shape, binary_t=False, S=2, seed=0):
    return cases.gpslc_object(gp, _case(n, shape, binary_t, S, seed))


def _levels(form, L):
    lv = nr.pairs(form, L)
    return lv, np.array([a for a, _ in lv]), (np.array([b for _, b in lv]) if form == "contrast" else None)


def _call(g, m, Xn, Un, form, doT, base, W, want=("mean", "var", "cov"), pred_noise=PN):
    return g.ctx().predict_new_weighted(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form,
                                        doT, base, W, pred_noise, want=want)


def _check(got, exp, W, case, what, samples=None):
    """(mean, var, cov or None) of the library against the literal dict, required then tight; `samples`: those only"""
    idx = list(range(case["S"])) if samples is None else list(samples)
    got = [None if a is None else a[idx] for a in got]
    ref = [None if exp[k] is None else exp[k][idx] for k in ("mean", "var", "cov")]
    na.check(got, ref, W, case["yScale"][idx], what, tight=False)
    na.check(got, ref, W, case["yScale"][idx], what, tight=True, worst=WORST)
    print(what, "worst error / tight bound so far:", WORST)


# ---- 1. against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("m", [1, 5, 128, 129, 300])
@pytest.mark.parametrize("n", [24, 129, 200])
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_against_restatement(gp, shape, n, m, form):
    """G = 6 weight columns in one call; L = 1 without the joint covariance (7 right-hand sides: 16 live rows) and L = 5 with it
    (31: 32 live rows); one new individual, a second row block with one live row, more row blocks than the factor has tiles"""
    c, g = _case(n, shape), _object(gp, n, shape)
    Xn, Un = nr.new_individuals(c, m, seed=m)
    W = na.weight_set(m, seed=n)
    for L, want_cov in ((1, False), (5, True)):
        lv, doT, base = _levels(form, L)
        st, mean, var, cov = _call(g, m, Xn, Un, form, doT, base, W, want=("mean", "var") + (("cov",) if want_cov else ()))
        assert st == 0 and mean.shape == var.shape == (2, L, 6) and (cov is None) == (not want_cov)
        _check((mean, var, cov), na.expected(c, Xn, Un, m, form, lv, W, want_cov=want_cov), W, c, f"L={L}")


@pytest.mark.parametrize("L,G", [(5, 3), (4, 4), (31, 1), (4, 8), (16, 8), (1, 65), (2, 127)])
@pytest.mark.parametrize("form", nr.FORMS)
def test_right_hand_side_counts_and_weight_column_passes(gp, form, L, G):
    """L G + 1 = 16, 17, 32, 33, 129 right-hand sides: both live-row layouts, a full augmented tile row and a second one; G = 65
    and 127: the second pass of the pair kernels over the weight columns"""
    n, m = 129, 130
    c, g = _case(n, "UX"), _object(gp, n, "UX")
    Xn, Un = nr.new_individuals(c, m, seed=L + G)
    W = na.many_weights(m, G, seed=L)
    lv, doT, base = _levels(form, L)
    st, mean, var, cov = _call(g, m, Xn, Un, form, doT, base, W)
    assert st == 0 and cov.shape == (2, L, L, G)
    _check((mean, var, cov), na.expected(c, Xn, Un, m, form, lv, W), W, c, f"L={L} G={G}")


@pytest.mark.parametrize("form", nr.FORMS)
def test_binary_treatment_through_the_c_entry_point(gp, form):
    n, S, m, L, G = 129, 2, 5, 3, 6
    c = cases.make_case(n, "UX", True, S=S, seed=122)
    g = cases.gpslc_object(gp, c)
    Xn, Un = nr.new_individuals(c, m, seed=3)
    lv = [(0.0, 1.0), (1.0, 0.0), (0.5, 0.2)] if form == "contrast" else [(0.0, None), (1.0, None), (0.5, None)]
    doT = np.array([a for a, _ in lv])
    base = np.array([b for _, b in lv]) if form == "contrast" else None
    W = na.weight_set(m)                                             # (G, m) C-contiguous: weights[i + m*g]
    mean, var, cov = np.empty((S, L, G), order="F"), np.empty((S, L, G), order="F"), np.empty((S, L, L, G), order="F")
    ctx = g.ctx()
    st = ctx.lib.gpslc_predict_new_weighted(ctx.h, S, *g._params(), m, _p(Xn), _p(Un), gp.api.NEW_FORMS[form], L, _p(doT), _p(base),
                                            G, _p(W), PN, _p(mean), _p(var), _p(cov))
    assert st == 0
    _check((mean, var, cov), na.expected(c, Xn, Un, m, form, lv, W), W, c, form)


# ---- 2. feature widths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("nU,nX", nw.ONE_PER_RUNG, ids=[f"F{u + x}" for u, x in nw.ONE_PER_RUNG])
def test_every_rung_of_the_feature_ladder(gp, nU, nX, form):
    """n = 129, m = 130 with the lengthscales rescaled so that kernel values are of order 1 at every width"""
    c = nw.width_case(nU, nX)
    Xn, Un = nw.width_new(nU, nX)
    assert nw.median_kernel(c, 0, Xn, Un) > 1e-3
    g = cases.gpslc_object(gp, c)
    W = na.weight_set(nw.M, seed=nU)
    lv, doT, base = nw.levels(form)
    st, mean, var, cov = _call(g, nw.M, Xn, Un, form, doT, base, W)
    assert st == 0
    _check((mean, var, cov), na.expected(c, Xn, Un, nw.M, form, lv, W), W, c, f"F={nU + nX} rung {nw.freg_rung(nU + nX)}")


# ---- 3. GPU against GPU, tight bounds -------------------------------------------------------------------------------------
KW = [dict(), dict(baseline=-0.3), dict(slope=True)]
KW_IDS = ["outcome", "contrast", "slope"]


@pytest.mark.parametrize("kw", KW, ids=KW_IDS)
def test_unit_vectors_and_quadratic_forms_against_predict_new(gp, kw):
    """w = e_i against predictNew's mean[i], var[i]; every weight vector against w' mean and w' cov w of predictNew(want_cov=True)"""
    n, m = 200, 129
    c, g = _case(n, "UX"), _object(gp, n, "UX")
    Xn, _ = nr.new_individuals(c, m, seed=11)
    like = np.arange(m) % n
    doTs = [0.6, -0.4]
    pm, pv, pc = gp.predictNew(g, doTs, Xnew=Xn, like=like, want_cov=True, **kw)          # (m, S, L), (S, L, m, m)
    units = [0, 5, 127, 128]
    E = np.zeros((len(units), m))
    E[np.arange(len(units)), units] = 1.0
    mean, var = gp.averageNew(g, doTs, Xnew=Xn, like=like, weights=E, **kw)
    exp = dict(mean=np.transpose(pm[units], (1, 2, 0)), var=np.transpose(pv[units], (1, 2, 0)), cov=None)
    _check((mean, var, None), exp, E, c, "unit vectors")
    W = na.weight_set(m)
    mean, var = gp.averageNew(g, doTs, Xnew=Xn, like=like, weights=W, **kw)
    exp = dict(mean=np.einsum("gi,isl->slg", W, pm), var=np.einsum("gi,slij,gj->slg", W, pc, W), cov=None)
    _check((mean, var, None), exp, W, c, "w' cov w")


@pytest.mark.parametrize("kw", KW, ids=KW_IDS)
def test_every_training_individual_copied_against_the_weighted_call(gp, kw):
    """Xnew = X, Unew = U (m = n): predict(weights=) and effectCurve of the training individuals.  The rows bw* are then
    wsum_mfma_kernel's to the bits and so are the means; beta comes from the MFMA where the weighted call sums w . bw, so the
    variances and covariances agree inside the tight bounds"""
    n = 200
    c, g = _case(n, "UX"), _object(gp, n, "UX")
    W = na.weight_set(n, seed=1)
    doTs = [0.6, -0.4, 1.1]
    pkw = dict(kw) if kw else dict(outcome=True)
    tm, tv = gp.predict(g, doTs, weights=W, **pkw)[:2]
    cm, cc = gp.effectCurve(g, doTs, weights=W, **pkw)
    mean, var, cov = gp.averageNew(g, doTs, Xnew=c["X"], Unew=c["U"], weights=W, want_cov=True, **kw)
    print("means bit-identical:", np.array_equal(mean, tm), " variances:", np.array_equal(var, tv), " covariances:", np.array_equal(cov, cc))
    _check((mean, var, cov), dict(mean=tm, var=tv, cov=cc), W, c, "copies")
    assert np.array_equal(cm, tm) and np.array_equal(mean, tm)


def test_a_partition_adds_up_to_the_population_average(gp):
    n, m = 129, 300
    c, g = _case(n, "UX"), _object(gp, n, "UX")
    Xn, Un = nr.new_individuals(c, m, seed=12)
    labels = np.arange(m) % 7
    keys, Wg = gp.groupWeights(labels)
    mean, _ = gp.averageNew(g, [0.6, -0.4], Xnew=Xn, Unew=Un, weights=Wg)
    everyone, _ = gp.averageNew(g, [0.6, -0.4], Xnew=Xn, Unew=Un)
    share = np.array([(labels == k).sum() / m for k in keys])
    total = mean @ share
    bound = 1e-9 * np.abs(everyone) + 1e-13
    print("partition: max err / bound", float(np.max(np.abs(total - everyone) / bound)))
    assert everyone.shape == (2, 2) and np.all(np.abs(total - everyone) <= bound)


# ---- 4. exact identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_exact_identities(gp, shape):
    c, g = _case(200, shape), _object(gp, 200, shape)
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=4)
    W = na.weight_set(m)
    A = np.array([0.37, 0.6, 0.37, -1.2])       # two real contrasts among the equal pairs
    B = np.array([0.37, -0.3, 0.37, 0.5])
    st, mean, var, cov = _call(g, m, Xn, Un, "contrast", A, B, W)
    assert st == 0
    zero = 5                                     # the zero column
    assert not mean[:, :, zero].any() and not var[:, :, zero].any() and not cov[:, :, :, zero].any()
    w2 = np.sum(W * W, axis=1)
    for l in range(4):
        same = A[l] == B[l]
        live = [gi for gi in range(6) if gi != zero and W[gi].any()]
        assert (not mean[:, l, live].any()) == same
        if same:
            assert np.all(np.abs(var[:, l] - PN * w2) <= 1e-14 * PN * w2)
            off = [k for k in range(4) if k != l]
            assert not cov[:, l, off].any() and not cov[:, off, l].any()
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1, 3)))
    assert np.array_equal(np.einsum("sllg->slg", cov), var)


# ---- 5. bits --------------------------------------------------------------------------------------------------------------
def test_a_columns_results_do_not_depend_on_the_other_columns(gp):
    """one column alone (6 right-hand sides: 16 live rows), among 6 (31: 32 live rows), the columns permuted, among 20 (101: the
    whole augmented tile row): the same bits.  Among 30 (151 right-hand sides: a second augmented tile row, where the epilogue
    takes z . v and v . v from the Schur tiles and no longer from the rows, as in every weighted call) the tight bounds."""
    n, m, L = 200, 140, 5
    c, g = _case(n, "UX"), _object(gp, n, "UX")
    Xn, Un = nr.new_individuals(c, m, seed=5)
    lv, doT, base = _levels("contrast", L)
    W = na.many_weights(m, 30, seed=2)
    st, mean, var, cov = _call(g, m, Xn, Un, "contrast", doT, base, W[:6])
    assert st == 0
    for idx in ([4], [5, 3, 1, 0, 2, 4], list(range(20)), list(range(30))):
        st, mean2, var2, cov2 = _call(g, m, Xn, Un, "contrast", doT, base, W[idx])
        assert st == 0
        for k, gi in enumerate(idx):
            if gi >= 6:
                continue
            same = [np.array_equal(a2[..., k], a[..., gi]) for a2, a in ((mean2, mean), (var2, var), (cov2, cov))]
            print(len(idx), "columns, column", gi, "mean / var / cov bit-identical:", same)
            if L * len(idx) + 1 <= 128:
                assert all(same), (len(idx), gi)
        if L * len(idx) + 1 > 128:
            _check((mean2[..., :6], var2[..., :6], cov2[..., :6]), dict(mean=mean, var=var, cov=cov), W[:6], c, "among 30")


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    c = _case(200, "UX", S=3)
    m = 129
    Xn, Un = nr.new_individuals(c, m, seed=7)
    W = na.weight_set(m)
    lv, doT, base = _levels("slope", 3)
    ref = _call(cases.gpslc_object(gp, c), m, Xn, Un, "slope", doT, base, W)
    assert ref[0] == 0
    for tuning in (dict(max_batch=1), dict(n_streams=2), dict(max_batch=1, n_streams=2)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            got = _call(g, m, Xn, Un, "slope", doT, base, W)
            assert got[0] == 0
            for x, y in zip(ref[1:], got[1:]):
                assert np.array_equal(x, y), (tuning, rep)
    _check(ref[1:], na.expected(c, Xn, Un, m, "slope", lv, W, samples=(2,)), W, c, "S = 3", samples=(2,))


def test_schedules_give_the_same_bits(gp):
    """five tiles: the factor and the right-hand-side rows from the persistent launch against the per-column schedule's"""
    from test_gpu_outcome import _forced_schedules
    c = _case(520, "UX")
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=8)
    W = na.weight_set(m)
    lv, doT, base = _levels("outcome", 2)
    out = _forced_schedules(gp, c, lambda g: _call(g, m, Xn, Un, "outcome", doT, base, W))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert out[0][0] == 0
    _check(out[0][1:], na.expected(c, Xn, Un, m, "outcome", lv, W, samples=(1,)), W, c, "five tiles", samples=(1,))


# ---- 6. each output alone, breakdown and argument errors ------------------------------------------------------------------
def test_each_output_alone(gp):
    c, g = _case(129, "UX"), _object(gp, 129, "UX")
    m = 130
    Xn, Un = nr.new_individuals(c, m, seed=9)
    W = na.weight_set(m)
    _, doT, base = _levels("contrast", 2)
    full = _call(g, m, Xn, Un, "contrast", doT, base, W)
    assert full[0] == 0
    for k, name in enumerate(("mean", "var", "cov"), start=1):
        one = _call(g, m, Xn, Un, "contrast", doT, base, W, want=(name,))
        assert one[0] == 0
        for j in range(1, 4):
            assert (one[j] is None) == (j != k)
        assert np.array_equal(one[k], full[k]), name


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
    W = na.weight_set(m)
    lv, doT, base = _levels("outcome", 2)
    st, mean, var, cov = _call(g, m, None, None, "outcome", doT, base, W)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for a in (mean, var, cov):
        assert np.isnan(a[0]).all() and np.isfinite(a[1]).all()
    _check((mean, var, cov), na.expected(c, None, None, m, "outcome", lv, W, samples=(1,)), W, c, "sample 1", samples=(1,))
    with pytest.raises(gp.PosDefException) as ei:
        gp.averageNew(g, doT)
    assert ei.value.info == 2


def test_argument_errors(gp):
    c = _case(24, "UX")
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    m = 3
    Xn, Un = nr.new_individuals(c, m)
    doT, base = np.array([0.6, 0.2]), np.array([0.1, 0.1])
    W = na.weight_set(m)

    def call(m=m, Xn=Xn, Un=Un, form="outcome", doT=doT, base=None, W=W, want=("mean", "var"), ctx=ctx, pred_noise=PN, **kw):
        return ctx.predict_new_weighted(2, g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, doT, base, W, pred_noise,
                                        want=want, **kw)[0]

    def message():
        return ctx.lib.gpslc_last_error(ctx.h).decode()

    assert call(m=0) == -9 and "argument #9" in message() and "m < 1" in message()
    assert call(doT=None) == -13 and "argument #13" in message() and "L < 1" in message()
    assert call(form=3) == -12 and "argument #12" in message() and "factual" in message()
    assert call(form="contrast") == -15 and "doT_base is NULL" in message()
    assert call(base=base) == -15 and "argument #15" in message() and "no contrast" in message()
    assert call(Xn=None) == -10 and "argument #10" in message() and "Xnew is NULL" in message()
    assert call(Un=None) == -11 and "argument #11" in message() and "Unew is NULL" in message()
    assert call(doT=np.array([0.6, np.nan])) == -14 and "argument #14" in message() and "non-finite" in message()
    assert call(G=0) == -16 and "argument #16" in message() and "G < 1" in message()
    assert call(W=None, G=2) == -17 and "argument #17" in message() and "weights is NULL" in message()
    bad = W.copy()
    bad[4, 1] = np.inf
    assert call(W=bad) == -17 and "non-finite" in message()
    assert call(pred_noise=np.nan) == -18 and "argument #18" in message()
    assert call(want=()) == -19 and "argument #19" in message() and "all NULL" in message()
    assert call() == 0                                                          # the context stays usable
    # an fp32 context
    g32 = cases.gpslc_object(gp, c, fp32_kernel=True)
    assert call(ctx=g32.ctx()) == -1007
    assert "fp64" in g32.ctx().lib.gpslc_last_error(g32.ctx().h).decode()
    assert np.isfinite(gp.predict(g32, doT)[0]).all()                           # and goes on serving what it supports
    fresh = gp.Context(24, 3, 2)
    assert call(ctx=fresh) == -1002                                             # GPSLC_ERR_NODATA
    assert call() == 0
