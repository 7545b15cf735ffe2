"""Leave-group-out predictive checks on the GPU (gpslc_y_lgo) against the host restatement (lgo_restatement.py).

Bound, per posterior sample: tol = max(1e-10, 1e-14 cond(A) max_g cond(C_g)) — the bound of test_gpu_loo.py for the entries of
W = L^-T, times the condition of the block C_g = inv(A)[I_g, I_g] that is then solved with.  lgoVar relative, lgoMean absolute
against tol max|Y|, lgoLpd absolute against tol (m_g + q_g) (m_g logarithms in the log determinant, q_g the refit's Mahalanobis
distance: the quadratic term).  Every comparison first asserts that the restatement's two computations (closed form, literal
refit) agree within the same bound; the device is then compared with the literal refit."""
import functools

import numpy as np
import pytest

import cases
import lgo_restatement as lg
from test_gpu_loo import _forced_schedules, _ill_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(n, shape, binary_t, S, seed):
    return cases.make_case(n, shape, binary_t, S=S, seed=seed)


def _labellings(n):
    out = {"singletons": lg.singletons(n), "mod7": lg.mod7(n), "blocks17": lg.blocks_of(n, 17)}
    if n <= 128:
        out["one group"] = lg.one_group(n)
    if n >= 136:
        out["rows 120..135"] = lg.with_block(n, 120, 136)
    if n >= 400:
        out["rows 100..227"] = lg.with_block(n, 100, 228)
    return out


@functools.lru_cache(maxsize=None)
def _expected(n, shape, binary_t, S, seed, name, samples=None):
    return lg.expected(_case(n, shape, binary_t, S, seed), _labellings(n)[name], samples=samples)


def _call(gp, g, labels, **kw):
    mean, var, lpd, keys = gp.lgoPredictive(g, groups=labels, **kw)
    assert np.array_equal(keys, np.arange(len(keys)))          # the test labellings are already compact
    return mean, var, lpd


def _check(exp, got, Y, labels, samples=None, tol=None, what=""):
    """got = (mean (n, S), var (n, S), lpd (G, S)) against exp[s]; tol=None: the sample's own bound"""
    for s in (exp if samples is None else samples):
        e = exp[s]
        t = e["tol"] if tol is None else tol
        host = lg.errors(e["closed"], e["refit"], e["q"], Y, labels)
        dev = lg.errors(tuple(a[:, s] for a in got), e["refit"], e["q"], Y, labels)
        print(what, "sample", s, "cond(A) %.3g cond(C) %.3g tol %.3g" % (e["cond"], e["cond_c"], t),
              "host (var, mean, lpd)", host, "device", dev)
        assert max(host) <= (e["tol"] if tol is None else min(tol, e["tol"])), ("host", what, s, host)
        assert max(dev) <= t, ("device", what, s, dev)


GRID = [(n, "UX", False) for n in (3, 128, 129, 200, 400)] + [(200, sh, False) for sh in ("U", "X", "T")] + [(200, "UX", True)]


@pytest.mark.parametrize("n,shape,binary_t", GRID)
def test_lgo_against_the_literal_refit(gp, n, shape, binary_t):
    """one tile with padding, an exact tile (one group of everybody: the full 128-row block), one live row in a second tile,
    two and four tiles; singletons, i mod 7 (scattered over the tile rows, sizes no multiple of 16 or 4), contiguous blocks of
    17, rows 120..135 across the tile boundary, at n = 400 a group of exactly 128 members in rows 100..227"""
    key = (n, shape, binary_t, 2, 60 + n)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    for name, labels in _labellings(n).items():
        got = _call(gp, g, labels)
        G = int(labels.max()) + 1
        assert got[0].shape == (n, 2) and got[1].shape == (n, 2) and got[2].shape == (G, 2)
        _check(_expected(*key, name), got, c["Y"], labels, what=f"n={n} {shape} bin={binary_t} {name}")
    assert not g.ctx().last_info(2).any()


def test_ill_conditioned_case(gp):
    c = _ill_case()
    labels = lg.mod7(200)
    exp = lg.expected(c, labels)
    for s in exp:
        assert 1e4 <= exp[s]["cond"] <= 1e8, exp[s]["cond"]
    _check(exp, _call(gp, cases.gpslc_object(gp, c), labels), c["Y"], labels, what="ill-conditioned")


# ---- identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 200])
def test_singletons_reproduce_leave_one_out(gp, n):
    key = (n, "UX", False, 2, 60 + n)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    labels = lg.singletons(n)
    got = _call(gp, g, labels)
    loo = gp.looPredictive(g)
    exp = _expected(*key, "singletons")
    for s in range(2):
        errs = lg.errors(tuple(a[:, s] for a in got), tuple(a[:, s] for a in loo), exp[s]["q"], c["Y"], labels)
        print("singletons against y_loo, sample", s, errs)
        assert max(errs) <= exp[s]["tol"], errs


@pytest.mark.parametrize("n", [3, 100, 128])
def test_one_group_of_everybody_is_the_prior(gp, n):
    """C = inv(A): lgoLpd = logpdf, lgoMean = 0 (the prior mean), lgoVar = diag(A)"""
    c = _case(n, "UX", False, 2, 60 + n)
    g = cases.gpslc_object(gp, c)
    labels = lg.one_group(n)
    mean, var, lpd = _call(gp, g, labels)
    logpdf = gp.yLogpdf(g)
    exp = lg.expected(c, labels)
    for s in range(2):
        e = exp[s]
        errs = lg.errors((mean[:, s], var[:, s], lpd[:, s]), (np.zeros(n), np.diag(e["A"]).copy(), logpdf[s:s + 1]), e["q"], c["Y"], labels)
        print("one group against the prior, n", n, "sample", s, "tol %.3g" % e["tol"], errs)
        assert max(errs) <= e["tol"], errs


# ---- bit identities ------------------------------------------------------------------------------------------------------
def test_renumbering_the_labels_permutes_lpd_only(gp):
    n = 200
    c = _case(n, "UX", False, 2, 60 + n)
    g = cases.gpslc_object(gp, c)
    for labels in (lg.mod7(n), lg.blocks_of(n, 17), lg.with_block(n, 120, 136)):
        G = int(labels.max()) + 1
        perm = np.random.default_rng(G).permutation(G).astype(np.int32)          # old label -> new label
        m0, v0, l0 = _call(gp, g, labels)
        m1, v1, l1 = _call(gp, g, perm[labels])
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        assert np.array_equal(l0, l1[perm, :])


def test_a_group_does_not_depend_on_how_the_others_are_grouped(gp):
    n = 400
    c = _case(n, "UX", False, 2, 60 + n)
    g = cases.gpslc_object(gp, c)
    a = lg.with_block(n, 120, 136, rest=17)                    # the group of rows 120..135 beside blocks of 17 ...
    b = lg.with_block(n, 120, 136, rest=5)                     # ... beside blocks of 5 ...
    d = np.where(a == a[120], 0, 1 + np.arange(n) % 3).astype(np.int32)          # ... and beside three scattered groups of ~128
    outs = [_call(gp, g, lab) for lab in (a, b, d)]
    I = np.arange(120, 136)
    for lab, (m, v, l) in zip((b, d), outs[1:]):
        assert np.array_equal(m[I], outs[0][0][I]) and np.array_equal(v[I], outs[0][1][I])
        assert np.array_equal(l[lab[120]], outs[0][2][a[120]])
    # a scattered group as well: i mod 7 == 3 inside i mod 7 and beside one-member groups
    e = lg.mod7(n)
    f = np.empty(n, dtype=np.int32)
    rest = np.flatnonzero(e != 3)
    f[rest] = 1 + np.arange(len(rest))
    f[e == 3] = 0
    (me, ve, le), (mf, vf, lf) = _call(gp, g, e), _call(gp, g, f)
    assert np.array_equal(me[e == 3], mf[e == 3]) and np.array_equal(ve[e == 3], vf[e == 3]) and np.array_equal(le[3], lf[0])


def test_schedules_give_the_same_bits(gp):
    """five tiles, S = 5: the factor and alpha from the persistent launch against the per-column schedule's"""
    key = (520, "UX", False, 5, 77)
    c = _case(*key)
    labels = lg.blocks_of(520, 17)
    labels[labels == labels.max()] = labels.max() - 1          # 520 = 30 x 17 + 10: the last ten join their neighbours (27)
    out = _forced_schedules(gp, c, lambda g: _call(gp, g, labels))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    _check(lg.expected(c, labels, samples=(4,)), out[0], c["Y"], labels, what="schedules")


def test_chunking_streams_and_repeats_give_the_same_bits(gp):
    n = 300
    c = _case(n, "UX", False, 5, 78)
    labels = lg.mod7(n)
    ref = _call(gp, cases.gpslc_object(gp, c), labels)
    for tuning in (dict(max_batch=2), dict(n_streams=1), dict(n_streams=3), dict(max_batch=2, n_streams=3)):
        g = cases.gpslc_object(gp, c)
        g.ctx().set_tuning(**tuning)
        for rep in range(2):
            for x, y in zip(ref, _call(gp, g, labels)):
                assert np.array_equal(x, y), (tuning, rep)
    _check(lg.expected(c, labels, samples=(1,)), ref, c["Y"], labels, what="chunking")


# ---- other ---------------------------------------------------------------------------------------------------------------
def _args(g):
    return (g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)


def test_each_output_alone_and_logpdf_is_y_loos(gp):
    n = 200
    c = _case(n, "UX", False, 2, 60 + n)
    g = cases.gpslc_object(gp, c)
    labels = lg.blocks_of(n, 17)
    G = int(labels.max()) + 1
    full = g.ctx().y_lgo(2, *_args(g), G, labels)
    assert full[0] == 0
    for k, name in enumerate(("mean", "var", "lpd"), start=1):
        one = g.ctx().y_lgo(2, *_args(g), G, labels, want=(name,))
        assert one[0] == 0
        for j in range(1, 5):
            assert (one[j] is None) == (j != k)
        assert np.array_equal(one[k], full[k]), name
    # lgoLpd beside logpdf (no LOO output is asked anywhere in this call)
    st, _, _, lpd, logpdf = g.ctx().y_lgo(2, *_args(g), G, labels, want=("lpd", "logpdf"))
    assert st == 0 and np.array_equal(lpd, full[3]) and np.array_equal(logpdf, full[4])
    loo = g.ctx().y_loo(2, *_args(g))
    assert loo[0] == 0 and np.array_equal(full[4], loo[4])     # the same factorisation: bit-identical
    # and the LOO call between two LGO calls changes nothing
    again = g.ctx().y_lgo(2, *_args(g), G, labels)
    for x, y in zip(full[1:], again[1:]):
        assert np.array_equal(x, y)


def test_overrides_against_the_literal_refit(gp):
    n = 200
    key = (n, "UX", False, 2, 60 + n)
    c = _case(*key)
    g = cases.gpslc_object(gp, c)
    labels = lg.mod7(n)
    rng = np.random.default_rng(5)
    Y2 = rng.standard_normal(n) * 2.0 + 1.0
    X2 = c["X"] + 0.3 * rng.standard_normal(c["X"].shape)
    _check(lg.expected(c, labels, Y=Y2), _call(gp, g, labels, Y_override=Y2), Y2, labels, what="Y override")
    _check(lg.expected(c, labels, X=X2), _call(gp, g, labels, X_override=X2), c["Y"], labels, what="X override")
    _check(lg.expected(c, labels, X=X2, Y=Y2), _call(gp, g, labels, X_override=X2, Y_override=Y2), Y2, labels, what="both overrides")
    # the context's own data afterwards: nothing of the overrides is kept
    _check(_expected(*key, "mod7"), _call(gp, g, labels), c["Y"], labels, what="after the overrides")
    s = gp.lgoSummary(g, groups=labels, Y_override=Y2)
    m, v, l = _call(gp, g, labels, Y_override=Y2)
    assert np.array_equal(s["zscore"], (Y2[:, None] - m) / np.sqrt(v)) and np.array_equal(s["elpd"], l.sum(axis=0))


def test_fp32_context_against_the_fp64_restatement(gp):
    """the bound of test_fp32_kernel_mode_drift_and_identities: 1e-6"""
    n = 300
    c = _case(n, "UX", False, 2, 85)
    labels = lg.blocks_of(n, 17)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    _check(lg.expected(c, labels), _call(gp, g, labels), c["Y"], labels, tol=1e-6, what="fp32")


def test_breakdown_gives_nan_for_that_sample_only(gp):
    """the case of test_gpu_loo.py: yNoise = 0 and a duplicated individual in a model without U and X — sample 0's matrix is
    singular (pivot 2 is exactly 0); an ordinary error return"""
    n = 200
    c = dict(cases.make_case(n, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    g = cases.gpslc_object(gp, c)
    labels = lg.mod7(n)
    st, mean, var, lpd, logpdf = g.ctx().y_lgo(2, None, None, None, None, None, g.tyLS, g.yScale, g.yNoise, 7, labels)
    assert st == 2
    assert list(g.ctx().last_info(2)) == [2, 0]
    for a in (mean, var, lpd):
        assert np.isnan(a[:, 0]).all()
    _check(lg.expected(c, labels, samples=(1,)), (mean, var, lpd), c["Y"], labels, what="beside a breakdown")
    with pytest.raises(gp.PosDefException) as ei:
        gp.lgoPredictive(g, groups=labels)
    assert ei.value.info == 2
    # the context keeps working
    c["yNoise"] = np.array([c["yNoise"][1], c["yNoise"][1]])
    g2 = cases.gpslc_object(gp, c)
    g2._ctx = g.ctx()
    assert np.isfinite(np.concatenate([a.ravel() for a in _call(gp, g2, labels)])).all()


def test_argument_errors(gp):
    n = 24
    c = _case(n, "UX", False, 2, 86)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    args = _args(g)
    good = lg.blocks_of(n, 5)                                  # 5 groups
    err = lambda: ctx.lib.gpslc_last_error(ctx.h)              # noqa: E731
    assert ctx.y_lgo(2, *args, 0, good)[0] == -11              # G < 1
    assert ctx.y_lgo(2, *args, n + 1, good)[0] == -11          # G > n
    assert ctx.y_lgo(2, *args, 5, None)[0] == -12              # labels NULL
    assert b"NULL" in err()
    bad = good.copy()
    bad[3] = 5
    assert ctx.y_lgo(2, *args, 5, bad)[0] == -12               # a label outside [0, G)
    bad[3] = -1
    assert ctx.y_lgo(2, *args, 5, bad)[0] == -12
    assert b"outside" in err()
    assert ctx.y_lgo(2, *args, 6, good)[0] == -12              # group 5 has no member
    assert b"no member" in err()
    assert ctx.y_lgo(2, *args, 5, good, want=("logpdf",))[0] == -13          # the three LGO outputs all NULL
    assert ctx.y_lgo(-1, *args, 5, good)[0] == -2              # gpslc_y_loo's checks and numbering come first
    assert ctx.y_lgo(2, None, *args[1:], 5, good)[0] == -3
    st, mean, var, lpd, logpdf = ctx.y_lgo(0, *args, 5, good)  # an empty call
    assert st == 0 and mean.shape == (n, 0) and lpd.shape == (5, 0)
    fresh = gp.Context(n, 3, 2)
    assert fresh.y_lgo(2, *args, 5, good)[0] == -1002          # GPSLC_ERR_NODATA: before set_data
    assert ctx.y_lgo(2, *args, 5, good)[0] == 0                # and the good call still runs
    # a group of 129 members
    c2 = _case(200, "UX", False, 2, 60 + 200)
    g2 = cases.gpslc_object(gp, c2)
    big = np.r_[np.zeros(60), np.ones(129), np.full(11, 2)].astype(np.int32)
    ctx2 = g2.ctx()
    st = ctx2.y_lgo(2, *_args(g2), 3, big)[0]
    with pytest.raises(gp.GPSLCError) as ei:
        ctx2.check(st)
    assert st != 0 and "group 1" in str(ei.value) and "129" in str(ei.value)
    with pytest.raises(gp.GPSLCError):
        gp.lgoPredictive(g2, groups=big)
    big[60] = 0                                                # 128: the largest group the call takes
    assert ctx2.y_lgo(2, *_args(g2), 3, big)[0] == 0


def test_lgo_predictive_uses_the_objects_of_prepare_data(gp):
    """an object built the way gpslc() builds it — prepareData sorts the rows by `obj`, the object keeps the column — gives the
    objects' leave-group-out checks with groups=None, the keys in sorted order"""
    from causalgpslc_jl_amd import inference
    n = 60
    c = _case(n, "UX", False, 2, 87)
    obj = np.repeat(np.arange(12), 5)                          # make_case's objects: five members each
    shuffle = np.random.default_rng(1).permutation(n)
    names = np.array(["h%02d" % (11 - o) for o in obj])       # string keys whose sorted order reverses the objects
    cols = {"T": c["T"][shuffle], "Y": c["Y"][shuffle], "obj": names[shuffle]}
    for k in range(c["X"].shape[1]):
        cols["x%d" % k] = c["X"][shuffle, k]
    SigmaU, sobj, X, T, Y = inference.prepareData(cols)
    order = shuffle[np.argsort(names[shuffle], kind="stable")]
    assert np.array_equal(Y, c["Y"][order]) and list(sobj) == list(names[order])
    g = gp.GPSLCObject(X, T, Y, np.asfortranarray(c["U"][order]), c["uyLS"], c["xyLS"], c["tyLS"], c["yNoise"], c["yScale"])
    with pytest.raises(ValueError, match="obj"):
        gp.lgoPredictive(g)                                    # no obj column yet
    g.obj = sobj
    mean, var, lpd, keys = gp.lgoPredictive(g)
    assert list(keys) == ["h%02d" % k for k in range(12)] and lpd.shape == (12, 2)
    labels = np.repeat(np.arange(12), 5).astype(np.int32)      # sorted by key: contiguous blocks of five
    sorted_case = dict(c, X=X, T=T, Y=Y, U=np.asfortranarray(c["U"][order]))
    _check(lg.expected(sorted_case, labels), (mean, var, lpd), Y, labels, what="objects")
    s = gp.lgoSummary(g)
    assert np.array_equal(s["elpd"], lpd.sum(axis=0)) and list(s["keys"]) == list(keys)
