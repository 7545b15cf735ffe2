"""K-fold cross-validation on the GPU (gpslc_y_kfold) against the host restatement (lgo_restatement.py): groups
of any size, the larger ones through the tiled factorisation of C = inv(A)[I, I].

Bound, per posterior sample: tests/test_gpu_lgo.py's, tol = max(1e-10, 1e-14 cond(A) max_g cond(C_g)) with its three error
measures (lgo_restatement.errors).  Every comparison first asserts that the restatement's two computations (closed form, literal
refit) agree within the bound; the device is then compared with the literal refit.  For the labellings here cond(A) <= 41 and
cond(C_g) <= 27 (tests/test_kfold.py): the bound is 1e-10 everywhere."""
import functools

import numpy as np
import pytest

import cases
import kfold_cases as kc
import lgo_restatement as lg
from test_gpu_lgo import _args, _check
from test_gpu_loo import _forced_schedules

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(n, S=2):
    return cases.make_case(n, "UX", False, S=S, seed=kc.SEEDS[n])


@functools.lru_cache(maxsize=None)
def _expected(n, name):
    return lg.expected(_case(n), kc.labellings(n)[name])


def _call(gp, g, labels, **kw):
    mean, var, lpd, keys = gp.kfoldPredictive(g, groups=labels, **kw)
    assert np.array_equal(keys, np.arange(len(keys)))          # the test labellings are already compact
    return mean, var, lpd


def _raw(g, labels, S=2, fn="y_kfold", **kw):
    return getattr(g.ctx(), fn)(S, *_args(g), int(labels.max()) + 1, labels, **kw)


# ---- 1. against the literal refit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 640, 645])
def test_kfold_against_the_literal_refit(gp, n):
    """n = 300 (three tiles, the last ragged): everybody (mt = 3), two folds of 150 (mt = 2), three folds (all small), rows
    0..128 beside blocks of 17 (mt = 2 with one row in the second tile, small and large groups in one call); n = 640 (five tiles,
    no padding): everybody (mt = 5), folds of 320 and of 214 / 213 / 213, groups of 129 / 256 / 255 with members in all five tile
    rows, a group of 257 whose first member lies in tile row 2; n = 645: five folds of 129"""
    c = _case(n)
    g = cases.gpslc_object(gp, c)
    for name, labels in kc.labellings(n).items():
        got = _call(gp, g, labels)
        G = int(labels.max()) + 1
        assert got[0].shape == (n, 2) and got[1].shape == (n, 2) and got[2].shape == (G, 2)
        assert all(np.isfinite(a).all() for a in got), name
        _check(_expected(n, name), got, c["Y"], labels, what=f"n={n} {name}")
        assert not g.ctx().last_info(2).any()


# ---- 2. small groups only: gpslc_y_lgo's bits ----------------------------------------------------------------------------
def test_small_groups_are_y_lgos_bit_for_bit(gp):
    n = 300
    g = cases.gpslc_object(gp, _case(n))
    for labels in (lg.mod7(n), lg.blocks_of(n, 17), lg.with_block(n, 100, 228)):
        a, b = _raw(g, labels), _raw(g, labels, fn="y_lgo")
        assert a[0] == 0 and b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y)


# ---- 3. bit invariance of a large group -----------------------------------------------------------------------------------
def test_a_large_group_does_not_depend_on_labels_or_on_the_other_groups(gp):
    n = 640
    g = cases.gpslc_object(gp, _case(n))
    I = kc.late_group()
    a, b = lg.beside(n, I, 1), lg.beside(n, I, 17)             # beside singletons, beside blocks of 17
    perm = np.random.default_rng(9).permutation(int(b.max()) + 1).astype(np.int32)          # old label -> new label
    (ma, va, la), (mb, vb, lb), (mp, vp, lp) = _call(gp, g, a), _call(gp, g, b), _call(gp, g, perm[b])
    assert np.array_equal(ma[I], mb[I]) and np.array_equal(va[I], vb[I]) and np.array_equal(la[0], lb[0])
    assert np.array_equal(mb, mp) and np.array_equal(vb, vp) and np.array_equal(lb, lp[perm, :])


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    n = 640
    c = _case(n, S=5)
    labels = kc.labellings(n)["129/256/255 dealt"]
    ref = _call(gp, cases.gpslc_object(gp, c), labels)
    for tuning in (dict(max_batch=2), dict(n_streams=1), dict(n_streams=3), dict(max_batch=2, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            for x, y in zip(ref, _call(gp, g, labels)):
                assert np.array_equal(x, y), (tuning, rep)
    _check(lg.expected(c, labels, samples=(3,)), ref, c["Y"], labels, what="chunking")


def test_schedules_give_the_same_bits(gp):
    """the factor of A and alpha from the persistent launch against the per-column schedule's; C takes the panels either way"""
    n = 640
    c = _case(n, S=5)
    labels = kc.labellings(n)["257 late"]
    out = _forced_schedules(gp, c, lambda g: _call(gp, g, labels))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_more_pairs_than_a_sub_batch_holds(gp):
    """five tiles: a sub-batch holds 128 (group, sample) pairs; 3 large groups x 44 samples = 132 pairs against the same samples
    four at a time"""
    n, S = 640, 44
    c = cases.make_case(n, "UX", False, S=S, seed=kc.SEEDS[n])
    labels = kc.labellings(n)["129/256/255 dealt"]
    g = cases.gpslc_object(gp, c)
    mean, var, lpd = _call(gp, g, labels)
    for s0 in (0, 20, 40):
        sub = dict(c, S=4)
        for k in ("U", "uyLS", "xyLS"):
            sub[k] = np.asfortranarray(c[k][..., s0:s0 + 4])
        for k in ("tyLS", "yScale", "yNoise"):
            sub[k] = c[k][s0:s0 + 4].copy()
        m4, v4, l4 = _call(gp, cases.gpslc_object(gp, sub), labels)
        assert np.array_equal(m4, mean[:, s0:s0 + 4]) and np.array_equal(v4, var[:, s0:s0 + 4]) and np.array_equal(l4, lpd[:, s0:s0 + 4])


# ---- 4. one group of everybody -----------------------------------------------------------------------------------------------
def test_one_group_of_everybody_is_the_prior(gp):
    """C = inv(A): cvLpd = logpdf, cvMean = 0 (the prior mean), cvVar = diag(A)"""
    n = 640
    c = _case(n)
    g = cases.gpslc_object(gp, c)
    labels = lg.one_group(n)
    st, mean, var, lpd, logpdf = _raw(g, labels)
    assert st == 0
    exp = _expected(n, "everybody")
    for s in range(2):
        e = exp[s]
        errs = lg.errors((mean[:, s], var[:, s], lpd[:, s]), (np.zeros(n), np.diag(e["A"]).copy(), logpdf[s:s + 1]), e["q"], c["Y"], labels)
        print("one group against the prior, sample", s, "tol %.3g" % e["tol"], errs)
        assert max(errs) <= e["tol"], errs


# ---- 5. continuity at the limit -----------------------------------------------------------------------------------------------
def test_128_and_129_members_both_meet_the_refit(gp):
    n = 300
    c = _case(n)
    g = cases.gpslc_object(gp, c)
    rows = lg.edge_group(129)
    for m in (128, 129):
        labels = lg.beside(n, rows[:m], 17)
        _check(lg.expected(c, labels), _call(gp, g, labels), c["Y"], labels, what=f"{m} members")


# ---- 6. breakdown of A ---------------------------------------------------------------------------------------------------------
def test_breakdown_gives_nan_for_that_sample_only(gp):
    """the case of test_gpu_lgo.py: yNoise = 0 and a duplicated individual in a model without U and X — sample 0's matrix is
    singular (pivot 2 is exactly 0); with two large groups and small ones beside them"""
    n = 300
    c = dict(cases.make_case(n, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    labels = np.where(np.arange(n) < 260, np.arange(n) % 2, 2 + (np.arange(n) - 260) // 20).astype(np.int32)     # 130, 130, 20, 20
    st, mean, var, lpd, logpdf = g.ctx().y_kfold(2, None, None, None, None, None, g.tyLS, g.yScale, g.yNoise, 4, labels)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for a in (mean, var, lpd):
        assert np.isnan(a[:, 0]).all()
    _check(lg.expected(c, labels, samples=(1,)), (mean, var, lpd), c["Y"], labels, what="beside a breakdown")
    with pytest.raises(gp.PosDefException) as ei:
        gp.kfoldPredictive(g, groups=labels)
    assert ei.value.info == 2


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(gp):
    n = 24
    c = cases.make_case(n, "UX", False, S=2, seed=86)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    args = _args(g)
    good = lg.blocks_of(n, 5)                                  # 5 groups
    err = lambda: ctx.lib.gpslc_last_error(ctx.h)              # noqa: E731
    assert ctx.y_kfold(2, *args, 0, good)[0] == -11            # G < 1
    assert ctx.y_kfold(2, *args, n + 1, good)[0] == -11        # G > n
    assert ctx.y_kfold(2, *args, 5, None)[0] == -12            # labels NULL
    assert b"NULL" in err()
    bad = good.copy()
    bad[3] = 5
    assert ctx.y_kfold(2, *args, 5, bad)[0] == -12             # a label outside [0, G)
    bad[3] = -1
    assert ctx.y_kfold(2, *args, 5, bad)[0] == -12
    assert b"outside" in err()
    assert ctx.y_kfold(2, *args, 6, good)[0] == -12            # group 5 has no member
    assert b"no member" in err()
    assert ctx.y_kfold(2, *args, 5, good, want=("logpdf",))[0] == -13        # the three outputs all NULL
    assert ctx.y_kfold(-1, *args, 5, good)[0] == -2            # gpslc_y_loo's checks and numbering come first
    assert ctx.y_kfold(2, None, *args[1:], 5, good)[0] == -3
    st, mean, var, lpd, logpdf = ctx.y_kfold(0, *args, 5, good)              # an empty call
    assert st == 0 and mean.shape == (n, 0) and lpd.shape == (5, 0)
    fresh = gp.Context(n, 3, 2)
    assert fresh.y_kfold(2, *args, 5, good)[0] == -1002        # GPSLC_ERR_NODATA: before set_data
    assert ctx.y_kfold(2, *args, 5, good)[0] == 0              # and the good call still runs


# ---- 8. a group of 129 members -----------------------------------------------------------------------------------------------------
def test_a_group_of_129_members_succeeds_where_y_lgo_refuses(gp):
    c = cases.make_case(200, "UX", False, S=2, seed=260)
    g = cases.gpslc_object(gp, c)
    big = np.r_[np.zeros(60), np.ones(129), np.full(11, 2)].astype(np.int32)
    ctx = g.ctx()
    st = _raw(g, big, fn="y_lgo")[0]
    with pytest.raises(gp.GPSLCError) as ei:
        ctx.check(st)
    assert st != 0 and "group 1" in str(ei.value) and "129" in str(ei.value)
    with pytest.raises(gp.GPSLCError):
        gp.lgoPredictive(g, groups=big)
    out = _raw(g, big)
    assert out[0] == 0
    exp = lg.expected(c, big)
    _check(exp, out[1:4], c["Y"], big, what="129 members, y_kfold")
    _check(exp, _call(gp, g, big), c["Y"], big, what="129 members, kfoldPredictive")


# ---- 9. fp32-kernel context ----------------------------------------------------------------------------------------------------------
def test_fp32_context_against_the_fp64_restatement(gp):
    """the bound of test_fp32_kernel_mode_drift_and_identities: 1e-6"""
    n = 640
    c = _case(n)
    labels = kc.labellings(n)["2 folds"]
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    _check(_expected(n, "2 folds"), _call(gp, g, labels), c["Y"], labels, tol=1e-6, what="fp32")


# ---- 10. the front end -----------------------------------------------------------------------------------------------------------------
def test_kfold_predictive_front_end(gp):
    n = 300
    c = _case(n)
    g = cases.gpslc_object(gp, c)
    folds = gp.foldLabels(n, 2, seed=5)
    mean, var, lpd, keys = gp.kfoldPredictive(g, K=2, seed=5)
    assert list(keys) == [0, 1] and lpd.shape == (2, 2)
    byg = gp.kfoldPredictive(g, groups=folds)
    assert all(np.array_equal(x, y) for x, y in zip((mean, var, lpd), byg[:3]))
    names = np.array(["fold b", "fold a"])[folds]              # string keys whose sorted order swaps the folds
    ms, vs, ls, ks = gp.kfoldPredictive(g, groups=names)
    assert list(ks) == ["fold a", "fold b"]
    assert np.array_equal(ms, mean) and np.array_equal(vs, var) and np.array_equal(ls, lpd[::-1])
    _check(lg.expected(c, folds), (mean, var, lpd), c["Y"], folds, what="K=2")
    with pytest.raises(ValueError, match="obj"):
        gp.kfoldPredictive(g)                                  # no obj column, neither argument
    with pytest.raises(ValueError, match="not both"):
        gp.kfoldPredictive(g, K=2, groups=folds)
    g.obj = names
    mo, vo, lo, ko = gp.kfoldPredictive(g)
    assert list(ko) == ["fold a", "fold b"] and np.array_equal(lo, ls) and np.array_equal(mo, ms)
    s = gp.kfoldSummary(g, K=2, seed=5)
    assert np.array_equal(s["elpd"], lpd.sum(axis=0)) and list(s["keys"]) == [0, 1]
    assert np.array_equal(s["zscore"], (c["Y"][:, None] - mean) / np.sqrt(var))
