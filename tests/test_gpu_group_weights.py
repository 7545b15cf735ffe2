"""Weighted average effects over groups (gpslc_predict_weighted and the Python mirror's `weights=`) against the dense
restatement in tests/weighted_restatement.py — w' MeanITE and w' (CovITE + pred_noise I) w from the oracle's n x n covariance —
and against the library's own unweighted outputs where an identity ties the two together.  Every test builds its reference
values on the host first and makes one library call per case.

Bounds (weighted_restatement.bounds), with ||w||_1 = sum |w_i|: the project's own for meanSATE / varSATE
(test_gpu_contrast._check) scaled so that w = 1/n reproduces them exactly (|w' Delta w| <= 4 yScale ||w||_1^2):
    required   |mean - ref| <= 1e-6 |ref| + 1e-12 ||w||_1     |var - ref| <= 1e-6 |ref| + 1e-9 yScale ||w||_1^2
    tight      |mean - ref| <= 1e-9 |ref| + 1e-13 ||w||_1     |var - ref| <= 1e-9 |ref| + 1e-12 yScale ||w||_1^2
"""
import ctypes as C

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import gpslc_oracle as orc
import weighted_restatement as wr

pytestmark = pytest.mark.gpu
PN = orc.PREDICTION_COVARIANCE_NOISE
GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


def _levels(c, L, con):
    """L levels (and baselines, for a contrast) of a case."""
    if con:
        return cr.pairs(c, L)
    lv = np.concatenate([c["doTs"][::-1], np.linspace(-1.1, 1.4, max(L - 2, 0))])[:L]
    return lv, None


def _check(exp, mw, vw, W, case, samples=None, mi=None):
    """Required, then tight bounds for every (sample, level, weight column); prints the worst error / tight bound."""
    worst_m = worst_v = 0.0
    S, L, G = mw.shape
    assert (L, G) == exp["mean"].shape[1:], (mw.shape, exp["mean"].shape)
    for s in (range(S) if samples is None else samples):
        for l in range(L):
            for g in range(G):
                rm, rv = exp["mean"][s, l, g], exp["var"][s, l, g]
                bm, bv, tm, tv = wr.bounds(rm, rv, W[g], case["yScale"][s])
                em, ev = abs(mw[s, l, g] - rm), abs(vw[s, l, g] - rv)
                worst_m, worst_v = max(worst_m, em / tm), max(worst_v, ev / tv)
                assert em <= bm, (s, l, g, mw[s, l, g], rm)
                assert ev <= bv, (s, l, g, vw[s, l, g], rv)
                assert em <= tm, (s, l, g, mw[s, l, g], rm, em / tm)
                assert ev <= tv, (s, l, g, vw[s, l, g], rv, ev / tv)
            if mi is not None:
                ref = exp["meanITE"][:, s, l]
                assert np.max(np.abs(mi[:, s, l] - ref)) <= 1e-9 * np.max(np.abs(ref)) + 1e-13, (s, l)
    print(f"worst error / tight bound: mean {worst_m:.3e} var {worst_v:.3e}")
    return worst_m, worst_v


# ---- 1. against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("con", [False, True])
@pytest.mark.parametrize("L", [1, 5])
def test_weighted_effects_against_restatement(gp, n, L, con, shape, bt):
    c = cases.make_case(n, shape, bt, S=2, seed=101 + L + n)
    lv, base = _levels(c, L, con)
    W = wr.weight_set(c, seed=n + L)
    exp = wr.expected_weighted(c, lv, W, base=base)
    mw, vw, mi = gp.predict(cases.gpslc_object(gp, c), lv, want_mean_ite=True, baseline=base, weights=W)
    assert mw.shape == vw.shape == (2, L, 7)
    _check(exp, mw, vw, W, c, mi=mi)


# ---- 2. layout switches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,G", [(3, 5), (2, 8), (1, 31), (4, 8), (1, 127), (2, 64), (2, 65), (1, 70)])
@pytest.mark.parametrize("con", [False, True])
def test_weighted_effects_where_the_right_hand_side_layout_switches(gp, L, G, con):
    """L G + 1 = 16 / 17, 32 / 33, 128 / 129 / 131 right-hand sides: 16 live rows, 32 live rows, a full augmented tile row, two
    tile rows; and G = 70, 127 (two passes of the weighted-sum kernel over the weight columns) — on two tiles per side."""
    c = cases.make_case(200, "UX", False, S=2, seed=135 + L * G)
    lv, base = _levels(c, L, con)
    W = wr.many_weights(c, G, seed=G)
    exp = wr.expected_weighted(c, lv, W, base=base)
    mw, vw, mi = gp.predict(cases.gpslc_object(gp, c), lv, want_mean_ite=True, baseline=base, weights=W)
    _check(exp, mw, vw, W, c, mi=mi)


# ---- 3. GPU against GPU: no restatement involved ----------------------------------------------------------------------
def _close(got, ref, w1, yscale=None):
    """The tight forms: mean (yscale None) or variance."""
    if yscale is None:
        return abs(got - ref) <= 1e-9 * abs(ref) + 1e-13 * w1
    return abs(got - ref) <= 1e-9 * abs(ref) + 1e-12 * yscale * w1 ** 2


@pytest.mark.parametrize("n,shape,bt", [(129, "UX", False), (200, "T", True), (400, "X", False)])
def test_unit_vector_is_one_individual_of_ite_distributions(gp, n, shape, bt):
    c = cases.make_case(n, shape, bt, S=2, seed=151 + n)
    g = cases.gpslc_object(gp, c)
    doT = float(c["doTs"][1])
    idx = [0, n // 3, n - 1]
    W = np.eye(n)[idx]
    M, CV = gp.ITEDistributions(g, doT)
    mw, vw, _ = gp.predict(g, [doT], weights=W)
    for s in range(c["S"]):
        for k, i in enumerate(idx):
            assert _close(mw[s, 0, k], M[s, i], 1.0), (s, i, mw[s, 0, k], M[s, i])
            assert _close(vw[s, 0, k], CV[s, i, i], 1.0, c["yScale"][s]), (s, i, vw[s, 0, k], CV[s, i, i])


@pytest.mark.parametrize("shape,bt", GRID8)
def test_uniform_weights_partitions_and_differences(gp, shape, bt):
    """w = 1/n is the plain call's meanSATE / varSATE; the group means of a partition average to meanSATE; the mean of a
    difference of two weight vectors is the difference of the means."""
    n = 200
    c = cases.make_case(n, shape, bt, S=3, seed=161)
    g = cases.gpslc_object(gp, c)
    lv = c["doTs"]
    labels = np.arange(n) // 5 % 7                      # seven groups of objects
    keys, Wg = gp.groupWeights(labels)
    cnt = np.array([(labels == k).sum() for k in keys])
    w1, w2 = wr.weight_set(c)[1], wr.weight_set(c)[6]
    W = np.vstack([np.full(n, 1.0 / n), Wg, w1, w2, w1 - w2])
    ms, vs, _ = gp.predict(g, lv)
    mw, vw, _ = gp.predict(g, lv, weights=W)
    for s in range(c["S"]):
        for l in range(len(lv)):
            assert _close(mw[s, l, 0], ms[s, l], 1.0), (s, l, mw[s, l, 0], ms[s, l])
            assert _close(vw[s, l, 0], vs[s, l], 1.0, c["yScale"][s]), (s, l, vw[s, l, 0], vs[s, l])
            part = float((cnt / n) @ mw[s, l, 1:8])
            assert _close(part, ms[s, l], 1.0), (s, l, part, ms[s, l])
            d = mw[s, l, 8] - mw[s, l, 9]
            assert _close(mw[s, l, 10], d, np.abs(w1 - w2).sum()), (s, l, mw[s, l, 10], d)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("n", [129, 400])
def test_att_of_a_binary_treatment_against_the_ordinary_levels(gp, n, shape):
    """f_i(1) - f_i(0) is -MeanITE_i(0) for the treated (their factual term is f_i(1)): the contrast (1, 0) weighted with the
    mask of the treated is minus the average of the ordinary call's MeanITE(0) over the treated — the ATT."""
    c = cases.make_case(n, shape, True, S=3, seed=143 + n)
    g = cases.gpslc_object(gp, c)
    treated = c["T"] == 1.0
    _, _, mi0 = gp.predict(g, [0.0], want_mean_ite=True)
    mw, vw, _ = gp.predict(g, [1.0], baseline=0.0, weights=treated)
    assert mw.shape == vw.shape == (3, 1)
    for s in range(c["S"]):
        ref = -float(np.mean(mi0[treated, s, 0]))
        assert _close(mw[s, 0], ref, 1.0), (s, mw[s, 0], ref)
        assert vw[s, 0] > 0.0


# ---- 4. exact results ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
def test_exact_zeros(gp, shape, bt):
    """A zero weight column: mean == 0.0 and var == 0.0.  A contrast level with a == b: mean == 0.0 and var == pred_noise w . w
    (to the rounding of w . w)."""
    n = 150
    c = cases.make_case(n, shape, bt, S=2, seed=121)
    g = cases.gpslc_object(gp, c)
    W = wr.weight_set(c)
    W[2] = 0.0
    a = 1.0 if bt else 0.37
    mw, vw, _ = gp.predict(g, [a, 0.0 if bt else -0.8], weights=W)
    assert np.all(mw[:, :, 2] == 0.0) and np.all(vw[:, :, 2] == 0.0)
    assert np.all(mw[:, :, 0] != 0.0) and np.all(vw[:, :, 0] > 0.0)
    mw, vw, _ = gp.predict(g, [a, a, 0.0 if bt else -0.8], baseline=[a, 0.0 if bt else -0.8, a], weights=W)
    ww = PN * np.sum(W * W, axis=1)
    assert np.all(mw[:, 0, :] == 0.0)
    assert np.all(np.abs(vw[:, 0, :] - ww) <= 1e-14 * ww)
    assert np.all(mw[:, :, 2] == 0.0) and np.all(vw[:, :, 2] == 0.0)
    keep = [0, 6]                                        # everyone, random weights: a real contrast is not zero
    assert np.all(mw[:, 1:, keep] != 0.0) and np.all(np.abs(vw[:, 1:, keep] - ww[keep]) > 1e-6 * ww[keep])


@pytest.mark.parametrize("shape,bt", GRID8)
def test_exact_zeros_when_every_treatment_equals_the_level(gp, shape, bt):
    """T_i == doT for every i (ordinary estimand): r == e == 1, so K w == B w bit for bit, c and w' Delta w vanish exactly."""
    n = 150
    c = cases.make_case(n, shape, bt, S=2, seed=123)
    t = 1.0 if bt else 0.7
    c["T"] = np.full(n, t)
    g = cases.gpslc_object(gp, c)
    W = wr.weight_set(c)
    mw, vw, _ = gp.predict(g, [t], weights=W)
    ww = PN * np.sum(W * W, axis=1)
    assert np.all(mw == 0.0)
    assert np.all(np.abs(vw[:, 0, :] - ww) <= 1e-14 * ww)


# ---- 5. bit-identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("con", [False, True])
def test_runs_and_chunkings_agree_bit_for_bit(gp, con):
    c = cases.make_case(200, "UX", False, S=7, seed=171)
    lv, base = _levels(c, 3, con)
    W = wr.weight_set(c)
    g = cases.gpslc_object(gp, c)
    first = gp.predict(g, lv, want_mean_ite=True, spp=4, seed=9, want_draws=True, baseline=base, weights=W)
    again = gp.predict(g, lv, want_mean_ite=True, spp=4, seed=9, want_draws=True, baseline=base, weights=W)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    g3 = cases.gpslc_object(gp, c)
    g3.ctx().set_tuning(max_batch=3)                     # 7 samples in chunks of 3, 3, 1
    chunked = gp.predict(g3, lv, want_mean_ite=True, spp=4, seed=9, want_draws=True, baseline=base, weights=W)
    for a, b in zip(first, chunked):
        assert np.array_equal(a, b)
    # MeanITE and the seeded draws are the unweighted call's
    plain = gp.predict(g, lv, want_mean_ite=True, spp=4, seed=9, want_draws=True, baseline=base)
    assert np.array_equal(first[2], plain[2]) and np.array_equal(first[3], plain[3])
    # and a single weight vector is column 0 of the array call
    one = gp.predict(g, lv, baseline=base, weights=W[3])
    assert one[0].shape == (7, 3) and np.array_equal(one[0], first[0][:, :, 3]) and np.array_equal(one[1], first[1][:, :, 3])


@pytest.mark.parametrize("L,con", [(3, False), (40, True)])
def test_weighted_effects_persistent_task_launch(gp, L, con):
    """The persistent launch forced down to one matrix (gpslc_set_task_schedule) really runs for a weighted call, and gives the
    per-column schedule's outputs bit for bit; both against the restatement."""
    c = cases.make_case(520, "UX", False, S=5, seed=141)
    lv, base = _levels(c, L, con)
    W = wr.weight_set(c)[:3]
    chk = [0, 4]
    exp = wr.expected_weighted(c, lv, W, base=base, samples=chk)
    out = []
    for tiles in (32, 0):
        g = cases.gpslc_object(gp, c)
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)      # HIP-event records: which schedule really ran
        g._ctx.set_data(g.X, g.T, g.Y)
        g.ctx().set_task_schedule(2, tiles, 1, 0)
        g.ctx().profile_reset()
        out.append(gp.predict(g, lv, want_mean_ite=True, baseline=base, weights=W))
        assert (g.ctx().profile_get(4)[0] > 0) == (tiles > 0)
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    _check(exp, out[0][0], out[0][1], W, c, samples=chk)


# ---- 6. public surface -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("con", [False, True])
def test_sate_distributions_and_sample_sate_take_the_weights(gp, con):
    n = 129
    c = cases.make_case(n, "UX", False, S=3, seed=181)
    g = cases.gpslc_object(gp, c)
    lv, base = _levels(c, 1, con)
    a, b = float(lv[0]), None if base is None else float(base[0])
    W = wr.weight_set(c)[[1, 3, 6]]
    exp = wr.expected_weighted(c, [a], W, base=None if b is None else [b])
    z = np.random.default_rng(182).standard_normal(c["S"] * 4)
    zg = np.random.default_rng(183).standard_normal((3, c["S"] * 4))
    m, v = gp.SATEDistributions(g, a, baseline=b, weights=W)
    m1, v1 = gp.SATEDistributions(g, a, baseline=b, weights=W[1])
    got1 = gp.sampleSATE(g, a, samplesPerPosterior=4, z=z, baseline=b, weights=W[1])
    gotg = gp.sampleSATE(g, a, samplesPerPosterior=4, z=zg, baseline=b, weights=W)
    seeded = gp.sampleSATE(g, a, samplesPerPosterior=4, seed=5, baseline=b, weights=W)
    assert m.shape == v.shape == (3, 3) and m1.shape == v1.shape == (3,)
    assert np.array_equal(m1, m[:, 1]) and np.array_equal(v1, v[:, 1])
    _check(exp, m[:, None, :], v[:, None, :], W, c)
    assert got1.shape == (12,) and gotg.shape == seeded.shape == (3, 12)
    assert np.allclose(got1, orc.sate_samples(exp["mean"][:, 0, 1], exp["var"][:, 0, 1], 4, z), rtol=1e-6, atol=1e-12)
    for k in range(3):
        assert np.allclose(gotg[k], orc.sate_samples(exp["mean"][:, 0, k], exp["var"][:, 0, k], 4, zg[k]), rtol=1e-6, atol=1e-12)
        assert np.array_equal(seeded[k], gp.SATEsamples(m[:, k], v[:, k], 4, seed=5 + k))


def test_fp32_context_refuses_weights(gp):
    c = cases.make_case(129, "UX", False, S=2, seed=191)
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    w = np.full(129, 1.0 / 129)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.SATEDistributions(g, 0.6, weights=w)
    assert ei.value.status == -1007 and "FP32" in str(ei.value)
    with pytest.raises(gp.GPSLCError) as ei:
        gp.predict(g, [0.6], baseline=-0.4, weights=w)
    assert ei.value.status == -1007
    gp.SATEDistributions(g, 0.6)               # the plain call of the same context keeps working


def test_vector_levels_refuse_weights(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=192)
    g = cases.gpslc_object(gp, c)
    g.ctx()
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, np.stack([c["T"] + 0.5]), weights=np.full(24, 1.0 / 24))


def test_c_argument_errors(gp):
    c = cases.make_case(24, "UX", False, S=2, seed=193)
    g = cases.gpslc_object(gp, c)
    ctx = g.ctx()
    lib = ctx.lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, S = 24, 2
    mw, vw = np.full((S, 2, 3), 7.0, order="F"), np.full((S, 2, 3), 7.0, order="F")
    ok = np.array([0.6, 0.1])
    W = np.ascontiguousarray(wr.weight_set(c)[:3])

    def call(L=2, doT=ok, base=None, G=3, w=W, spp=0, dr=None):
        return lib.gpslc_predict_weighted(ctx.h, S, *g._params(), L, p(doT), p(base), G, p(w), PN, spp, 0, None, p(mw), p(vw),
                                          None, p(dr))

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
    assert np.all(mw == 7.0) and np.all(vw == 7.0)          # nothing above wrote a result
    assert call() == 0 and call(base=ok[::-1].copy()) == 0
    exp = wr.expected_weighted(c, ok, W, base=ok[::-1])
    _check(exp, mw, vw, W, c)
