"""The joint covariance of weighted effects across the levels of one call (gpslc_predict_curve, effectCurve) against the
literal joint Gaussian process of tests/curve_restatement.py, against the structured restatement where the literal side
would be slow, and against the library's own outputs where an identity ties them together.

Bounds (weighted_restatement.bounds with the covariance entry in place of the variance), ||w||_1 = sum |w_i|:
    required   |mean - ref| <= 1e-6 |ref| + 1e-12 ||w||_1     |cov - ref| <= 1e-6 |ref| + 1e-9 yScale ||w||_1^2
    tight      |mean - ref| <= 1e-9 |ref| + 1e-13 ||w||_1     |cov - ref| <= 1e-9 |ref| + 1e-12 yScale ||w||_1^2
The required bounds are asserted; the worst error as a fraction of the tight bound is printed.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import curve_restatement as cu
import gpslc_oracle as orc
import weighted_restatement as wr

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


def _curve(gp, g, lv, base, W, **kw):
    """(meanW, varW, covW, meanITE, draws) of one gpslc_predict_curve call with a (G, n) weight array."""
    out, _ = gp.api._predict_curve(g, lv, baseline=base, weights=np.atleast_2d(W), **kw)
    return out


def _check(exp, mw, cw, W, case, samples=None):
    """Required bounds for every (sample, level pair, weight column); prints and returns the worst error / tight bound."""
    worst_m = worst_c = 0.0
    S, L, G = mw.shape
    assert cw.shape == (S, L, L, G) and exp["mean"].shape == mw.shape
    for s in (range(S) if samples is None else samples):
        for g in range(G):
            for l in range(L):
                rm = exp["mean"][s, l, g]
                bm, _, tm, _ = wr.bounds(rm, 0.0, W[g], case["yScale"][s])
                em = abs(mw[s, l, g] - rm)
                worst_m = max(worst_m, em / tm)
                assert em <= bm, (s, l, g, mw[s, l, g], rm)
                for lp in range(L):
                    rc = exp["cov"][s, l, lp, g]
                    _, bc, _, tc = wr.bounds(0.0, rc, W[g], case["yScale"][s])
                    ec = abs(cw[s, l, lp, g] - rc)
                    worst_c = max(worst_c, ec / tc)
                    assert ec <= bc, (s, l, lp, g, cw[s, l, lp, g], rc)
    print(f"worst error / tight bound: mean {worst_m:.3e} cov {worst_c:.3e}")
    return worst_m, worst_c


def _structured(case, lv, base, W, samples):
    S, L, G = case["S"], len(lv), W.shape[0]
    mean, cov = np.zeros((S, L, G)), np.zeros((S, L, L, G))
    for s in samples:
        for g in range(G):
            mean[s, :, g], cov[s, :, :, g] = cu.structured_curve(case, s, lv, W[g], base)
    return dict(mean=mean, cov=cov)


def _invariants(mw, vw, cw):
    """What holds for every call: exact symmetry, and the diagonal is varW to the bits."""
    assert np.array_equal(cw, np.transpose(cw, (0, 2, 1, 3)))
    L = mw.shape[1]
    for l in range(L):
        assert np.array_equal(cw[:, l, l, :], vw[:, l, :])
    assert np.all(np.isfinite(cw))


# ---- 1. against the literal joint GP ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("con", [False, True])
@pytest.mark.parametrize("L", [1, 5])
def test_curve_against_the_literal_joint_gp(gp, n, L, con, shape, bt):
    """One partial tile, tile edge + 1, two tiles, four tiles; L = 5 ends with a repeat of the first level."""
    c = cases.make_case(n, shape, bt, S=2, seed=201 + L + n)
    lv, base = cu.curve_levels(c, L, con)
    W = wr.weight_set(c, seed=n + L)
    exp = cu.expected_curve(c, lv, W, base)
    mw, vw, cw, _, _ = _curve(gp, cases.gpslc_object(gp, c), lv, base, W)
    _invariants(mw, vw, cw)
    _check(exp, mw, cw, W, c)


# ---- 2. right-hand-side counts -----------------------------------------------------------------------------------------
RHS = [(5, 3), (4, 4), (31, 1), (32, 1), (127, 1), (128, 1), (13, 10)]


def _sweep(c, L, con):
    """L distinct levels over the range of the treatment (a contrast: against baselines at least 0.25 away)."""
    if c["binary_t"]:
        return cu.curve_levels(c, L, con)
    lv = np.linspace(-1.6, 1.7, L)
    return (lv, lv - 0.3 - 0.4 * (np.arange(L) % 3)) if con else (lv, None)


@pytest.mark.parametrize("L,G", RHS)
@pytest.mark.parametrize("con", [False, True])
def test_right_hand_side_counts_one_partial_tile_literal(gp, L, G, con):
    """L G + 1 = 16 / 17 / 32 / 33 / 128 / 129 / 131 right-hand sides — 16 live rows, 32, a full augmented tile row, two tile
    rows — at n = 24 against the literal joint GP (sample 0; both samples for the short sweeps)."""
    c = cases.make_case(24, "UX", False, S=2, seed=211 + L * G)
    lv, base = _sweep(c, L, con)
    W = wr.many_weights(c, G, seed=G)
    chk = [0] if L > 40 else [0, 1]
    exp = cu.expected_curve(c, lv, W, base, samples=chk)
    mw, vw, cw, _, _ = _curve(gp, cases.gpslc_object(gp, c), lv, base, W)
    _invariants(mw, vw, cw)
    _check(exp, mw, cw, W, c, samples=chk)


@pytest.mark.parametrize("L,G", RHS)
@pytest.mark.parametrize("con", [False, True])
def test_right_hand_side_counts_two_tiles_structured(gp, L, G, con):
    """The same counts on two tiles per side against the structured restatement (tests/test_effect_curve.py holds it
    against the literal side)."""
    c = cases.make_case(200, "UX", False, S=2, seed=221 + L * G)
    lv, base = _sweep(c, L, con)
    W = wr.many_weights(c, G, seed=G)
    exp = _structured(c, lv, base, W, [0, 1])
    mw, vw, cw, _, _ = _curve(gp, cases.gpslc_object(gp, c), lv, base, W)
    _invariants(mw, vw, cw)
    _check(exp, mw, cw, W, c)


# ---- 3. GPU against GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("con", [False, True])
def test_other_outputs_are_the_weighted_calls_to_the_bits(gp, con):
    c = cases.make_case(200, "UX", False, S=3, seed=231)
    lv, base = cu.curve_levels(c, 4, con)
    W = wr.weight_set(c)
    g = cases.gpslc_object(gp, c)
    mw, vw, cw, mi, dr = _curve(gp, g, lv, base, W, want_mean_ite=True, spp=4, seed=9, want_draws=True)
    ref = gp.predict(g, lv, want_mean_ite=True, spp=4, seed=9, want_draws=True, baseline=base, weights=W)
    for a, b in zip((mw, vw, mi, dr), ref):
        assert np.array_equal(a, b)
    _invariants(mw, vw, cw)
    # covW == NULL is the weighted call; varW == NULL still gives the covariance its diagonal
    mw2, vw2, none, _, _ = _curve(gp, g, lv, base, W, want_cov=False)
    assert none is None and np.array_equal(mw2, mw) and np.array_equal(vw2, vw)
    ctx = g.ctx()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    Wc = np.ascontiguousarray(W)
    only = np.empty((3, 4, 4, 7), order="F")
    st = ctx.lib.gpslc_predict_curve(ctx.h, 3, *g._params(), 4, p(np.ascontiguousarray(lv)), p(base), 7, p(Wc), PN, 0, 0,
                                     None, None, None, p(only), None, None)
    assert st == 0 and np.array_equal(only, cw)
    # effectCurve / sampleEffectCurve: the public shapes
    m1, c1 = gp.effectCurve(g, lv, baseline=base, weights=W[3])
    assert m1.shape == (3, 4) and c1.shape == (3, 4, 4)
    assert np.array_equal(m1, mw[:, :, 3]) and np.array_equal(c1, cw[:, :, :, 3])
    mg, cg = gp.effectCurve(g, lv, baseline=base, weights=W)
    assert np.array_equal(mg, mw) and np.array_equal(cg, cw)
    m0, c0 = gp.effectCurve(g, lv, baseline=base)                      # weights=None: 1/n, the SATE curve
    ms, vs, _ = gp.predict(g, lv, baseline=base)
    for l in range(4):
        assert np.allclose(m0[:, l], ms[:, l], rtol=1e-9, atol=1e-13)
        assert np.allclose(c0[:, l, l], vs[:, l], rtol=1e-9, atol=1e-12 * np.max(c["yScale"]))
    z = np.random.default_rng(232).standard_normal((4, 5, 3))
    d1 = gp.sampleEffectCurve(g, lv, samplesPerPosterior=5, z=z, baseline=base, weights=W[3])
    assert d1.shape == (4, 15)
    ref1 = cu.curve_samples(mw[:, :, 3:4], cw[:, :, :, 3:4], 5, z[:, :, :, None])[:, :, :, 0]
    assert np.allclose(d1, ref1.reshape(4, 15, order="F"), rtol=1e-9, atol=1e-12)
    dg = gp.sampleEffectCurve(g, lv, samplesPerPosterior=5, seed=3, baseline=base, weights=W)
    assert dg.shape == (7, 4, 15) and np.array_equal(dg, gp.sampleEffectCurve(g, lv, 5, seed=3, baseline=base, weights=W))


@pytest.mark.parametrize("shape,bt", GRID8)
def test_exact_zeros(gp, shape, bt):
    """A zero weight column gives an all-0.0 block; a contrast level with a_l == b_l gives row and column l exactly 0.0 off
    the diagonal (and pred_noise w . w on it)."""
    n = 150
    c = cases.make_case(n, shape, bt, S=2, seed=241)
    g = cases.gpslc_object(gp, c)
    W = wr.weight_set(c)
    W[2] = 0.0
    a, b = (1.0, 0.0) if bt else (0.37, -0.8)
    mw, vw, cw, _, _ = _curve(gp, g, [a, b, 0.5 * (a + b)], None, W)
    _invariants(mw, vw, cw)
    assert np.all(cw[:, :, :, 2] == 0.0) and np.all(cw[:, :, :, 0] != 0.0)
    mw, vw, cw, _, _ = _curve(gp, g, [a, b, a, b], [b, b, a, a], W)
    _invariants(mw, vw, cw)
    assert np.all(cw[:, :, :, 2] == 0.0)
    for l in (1, 2):
        off = [k for k in range(4) if k != l]
        assert np.all(cw[:, l, off, :] == 0.0) and np.all(cw[:, off, l, :] == 0.0)
    keep = [0, 6]
    assert np.all(cw[:, 0, 3, keep] != 0.0)                            # f(a) - f(b) against f(b) - f(a): minus the variance
    ww = PN * np.sum(W * W, axis=1)
    for s in range(2):
        for j in keep:
            ref = -(vw[s, 0, j] - ww[j])
            _, bound, _, _ = wr.bounds(0.0, ref, W[j], c["yScale"][s])
            assert abs(cw[s, 0, 3, j] - ref) <= bound, (s, j, cw[s, 0, 3, j], ref)


@pytest.mark.parametrize("shape,bt", [("UX", False), ("X", False), ("T", False), ("U", False)])
def test_every_pair_of_an_ordinary_call_against_the_contrast_call(gp, shape, bt):
    """Var(tau_l - tau_l') = cov_ll + cov_l'l' - 2 cov_ll' (without the two levels' jitter) is the contrast (d_l, d_l')'s
    variance (without its own): the factual term cancels."""
    n = 200
    c = cases.make_case(n, shape, bt, S=2, seed=251)
    g = cases.gpslc_object(gp, c)
    W = wr.weight_set(c)
    lv = np.array([-0.9, -0.2, 0.45, 1.1])
    _, vw, cw, _, _ = _curve(gp, g, lv, None, W)
    pa = [(l, lp) for l in range(4) for lp in range(4) if l != lp]
    _, vc, _ = gp.predict(g, lv[[p[0] for p in pa]], baseline=lv[[p[1] for p in pa]], weights=W)
    ww = PN * np.sum(W * W, axis=1)
    for k, (l, lp) in enumerate(pa):
        for s in range(2):
            for j in range(7):
                got = cw[s, l, l, j] + cw[s, lp, lp, j] - 2.0 * cw[s, l, lp, j] - 2.0 * ww[j]
                ref = vc[s, k, j] - ww[j]
                _, bound, _, _ = wr.bounds(0.0, ref, W[j], c["yScale"][s])
                assert abs(got - ref) <= bound, (s, l, lp, j, got, ref)


# ---- 4. bit-identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,G,con", [(3, 7, False), (3, 7, True), (40, 4, False)])
def test_runs_chunkings_and_streams_agree_bit_for_bit(gp, L, G, con):
    c = cases.make_case(200, "UX", False, S=7, seed=261)
    lv, base = _sweep(c, L, con)
    W = wr.many_weights(c, G)
    g = cases.gpslc_object(gp, c)
    first = _curve(gp, g, lv, base, W, want_mean_ite=True)[:4]
    again = _curve(gp, g, lv, base, W, want_mean_ite=True)[:4]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    for tuning in (dict(max_batch=3, n_streams=1), dict(max_batch=3, n_streams=2)):      # 7 samples in chunks of 3, 3, 1
        g3 = cases.gpslc_object(gp, c)
        g3.ctx().set_tuning(**tuning)
        other = _curve(gp, g3, lv, base, W, want_mean_ite=True)[:4]
        for a, b in zip(first, other):
            assert np.array_equal(a, b), tuning


@pytest.mark.parametrize("L,con", [(3, False), (40, True)])
def test_curve_persistent_task_launch(gp, L, con):
    """The persistent launch forced down to one matrix really runs for a curve call and gives the per-column schedule's
    outputs bit for bit; sample 0 against the structured restatement."""
    c = cases.make_case(520, "UX", False, S=5, seed=271)
    lv, base = _sweep(c, L, con)
    W = wr.weight_set(c)[:3]
    out = []
    for tiles in (32, 0):
        g = cases.gpslc_object(gp, c)
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)      # HIP-event records: which schedule really ran
        g._ctx.set_data(g.X, g.T, g.Y)
        g.ctx().set_task_schedule(2, tiles, 1, 0)
        g.ctx().profile_reset()
        out.append(_curve(gp, g, lv, base, W, want_mean_ite=True)[:4])
        assert (g.ctx().profile_get(4)[0] > 0) == (tiles > 0)
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    _invariants(*out[0][:3])
    _check(_structured(c, lv, base, W, [0]), out[0][0], out[0][2], W, c, samples=[0])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_fp32_context_refuses_the_curve(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=281)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.effectCurve(g, [0.6, 0.1])
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.sampleEffectCurve(g, [0.6, 0.1], baseline=-0.4)
    assert ei.value.status == -1007
    gp.SATEDistributions(g, 0.6)               # the plain call of the same context keeps working


def test_c_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=291)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    lib = ctx.lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, S = 24, 2
    mw, vw = np.full((S, 2, 3), 7.0, order="F"), np.full((S, 2, 3), 7.0, order="F")
    cw = np.full((S, 2, 2, 3), 7.0, order="F")
    ok = np.array([0.6, 0.1])
    W = np.ascontiguousarray(wr.weight_set(c)[:3])

    def call(S_=S, L=2, doT=ok, base=None, G=3, w=W, spp=0, dr=None):
        return lib.gpslc_predict_curve(ctx.h, S_, *g._params(), L, p(doT), p(base), G, p(w), PN, spp, 0, None, p(mw), p(vw),
                                       p(cw), None, p(dr))

    assert call(S_=-1) == -2
    for bad in (np.array([0.6, np.nan]), np.array([np.inf, 0.1]), None):
        assert call(doT=bad) == -10 and "argument #10" in lib.gpslc_last_error(ctx.h).decode()
    for bad in (np.array([0.6, np.nan]), np.array([-np.inf, 0.1])):
        assert call(base=bad) == -11 and "argument #11" in lib.gpslc_last_error(ctx.h).decode()
    assert call(L=0) == -9
    assert call(G=0) == -12 and "argument #12" in lib.gpslc_last_error(ctx.h).decode()
    assert call(G=-1) == -12
    Wbad = W.copy()
    Wbad[2, 5] = np.nan
    assert call(w=Wbad) == -13 and "argument #13" in lib.gpslc_last_error(ctx.h).decode()
    Wbad[2, 5] = np.inf
    assert call(w=Wbad) == -13
    assert call(w=None) == -13
    assert call(dr=np.empty((2, n, S))) == -15 and "argument #15" in lib.gpslc_last_error(ctx.h).decode()
    assert np.all(mw == 7.0) and np.all(vw == 7.0) and np.all(cw == 7.0)          # nothing above wrote a result
    assert call(S_=0) == 0 and np.all(cw == 7.0)
    assert call() == 0
    exp = cu.expected_curve(c, ok, W)
    _check(exp, mw, cw, W, c)
    assert call(base=ok[::-1].copy()) == 0
    exp = cu.expected_curve(c, ok, W, ok[::-1])
    _check(exp, mw, cw, W, c)
