"""The joint covariance of weighted effects across intervention levels, without a GPU: the structured
formulas the library evaluates against the literal joint Gaussian process of tests/curve_restatement.py, that literal side
against the oracle's own CovITE, the host-only gpslc_curve_samples (pivoted Cholesky of semi-definite blocks), and the parsing
and refusals of effectCurve / sampleEffectCurve (all raised before any device call).

Bounds: weighted_restatement.bounds with the covariance entry in place of the variance,
    tight   |mean - ref| <= 1e-9 |ref| + 1e-13 ||w||_1      |cov - ref| <= 1e-9 |ref| + 1e-12 yScale ||w||_1^2
"""
import ctypes as C
import inspect

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import curve_restatement as cu
import gpslc_oracle as orc
import weighted_restatement as wr

GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]
EPS = np.finfo(np.float64).eps


# ---- the derivation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("con", [False, True])
@pytest.mark.parametrize("L", [1, 5])
def test_structured_formulas_against_the_literal_joint_gp(n, shape, bt, con, L):
    """Cov(tau_l, tau_l') = P_ll' - v_l . v_l' + [l == l'] pred_noise w . w reproduces w' CovITE_ll' w of the joint GP over all
    n (L + 1) (contrast: n (2 L + 1)) points for the seven weight vectors, inside the tight bounds; no block has a negative
    eigenvalue beyond rounding."""
    c = cases.make_case(n, shape, bt, S=1, seed=21 + n + L)
    Lv = 4 if (n == 400 and L == 5) else L
    lv, base = cu.curve_levels(c, Lv, con)
    W = wr.weight_set(c, seed=n + L)
    mean, cov = cu.literal_curve(c, 0, lv, W, base)
    worst_m = worst_c = 0.0
    for g in range(W.shape[0]):
        m, cv = cu.structured_curve(c, 0, lv, W[g], base)
        assert np.array_equal(cv, cv.T)
        for l in range(Lv):
            _, _, tm, _ = wr.bounds(mean[l, g], 0.0, W[g], c["yScale"][0])
            worst_m = max(worst_m, abs(m[l] - mean[l, g]) / tm)
            assert abs(m[l] - mean[l, g]) <= tm, (wr.WEIGHT_NAMES[g], l, m[l], mean[l, g])
            for lp in range(Lv):
                _, _, _, tv = wr.bounds(0.0, cov[l, lp, g], W[g], c["yScale"][0])
                worst_c = max(worst_c, abs(cv[l, lp] - cov[l, lp, g]) / tv)
                assert abs(cv[l, lp] - cov[l, lp, g]) <= tv, (wr.WEIGHT_NAMES[g], l, lp, cv[l, lp], cov[l, lp, g])
        ev = np.linalg.eigvalsh(cov[:, :, g])
        assert ev[0] >= -1e-12 * c["yScale"][0] * np.sum(np.abs(W[g])) ** 2, (wr.WEIGHT_NAMES[g], ev)
    print(f"worst error / tight bound: mean {worst_m:.2e} cov {worst_c:.2e}")


@pytest.mark.parametrize("shape,bt", [("UX", False), ("T", True), ("X", False)])
@pytest.mark.parametrize("con", [False, True])
def test_literal_diagonal_blocks_are_the_oracles_cov_ite(shape, bt, con):
    """The joint GP restricted to one level is ITEDistributions: CovITE_ll (symmetrised, + pred_noise I) of the literal side
    equals the oracle's (contrast: contrast_restatement's) to the rounding of evaluating the same expression twice
    (1e-10 of the largest entry), and the weighted diagonal equals weighted_restatement's."""
    n = 60
    c = cases.make_case(n, shape, bt, S=2, seed=31)
    lv, base = cu.curve_levels(c, 3, con)
    smp = cases.samples_of(c)
    W = wr.weight_set(c)
    expw = wr.expected_weighted(c, lv, W, base=base)
    for s in range(c["S"]):
        tv, pairs = cu._blocks(c["T"], lv, base)
        jg = cu.JointGP(smp[s], c["X"], c["T"], c["Y"], tv)
        for l in range(3):
            if con:
                M, Cv = cr.ite_distributions_contrast([smp[s]], c["X"], c["T"], c["Y"], lv[l], base[l])
            else:
                M, Cv = orc.ite_distributions([smp[s]], c["X"], c["T"], c["Y"], lv[l])
            blk = orc._symmetric_upper(cu.cov_ite_block(jg, pairs, l, l)) + np.eye(n) * cu.PN
            assert np.max(np.abs(blk - Cv[0])) <= 1e-10 * np.max(np.abs(Cv[0]))
            mi = jg.mean[pairs[l][0]] - jg.mean[pairs[l][1]]
            assert np.max(np.abs(mi - M[0])) <= 1e-10 * np.max(np.abs(M[0])) + 1e-13
        mean, cov = cu.literal_curve(c, s, lv, W, base)
        for l in range(3):
            for g in range(7):
                _, _, tm, tvv = wr.bounds(expw["mean"][s, l, g], expw["var"][s, l, g], W[g], c["yScale"][s])
                assert abs(mean[l, g] - expw["mean"][s, l, g]) <= tm
                assert abs(cov[l, l, g] - expw["var"][s, l, g]) <= tvv


def test_two_levels_are_correlated():
    """Why the per-level variances are not enough: the effects at two nearby levels share the Gaussian process."""
    c = cases.make_case(60, "UX", False, S=1, seed=5)
    _, cov = cu.literal_curve(c, 0, [0.5, 0.6], np.full((1, 60), 1 / 60))
    assert cov[0, 1, 0] > 0.9 * np.sqrt(cov[0, 0, 0] * cov[1, 1, 0])


# ---- gpslc_curve_samples: host only ----------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _factor(gp, cov):
    """F of every (s, g) block through z = identity: (L, L, S, G)."""
    S, L, _, G = cov.shape
    z = np.asfortranarray(np.broadcast_to(np.eye(L)[:, :, None, None], (L, L, S, G)))
    return gp.curveSamples(np.zeros((S, L, G)), cov, L, z=z)


def _random_psd(rng, L, rank):
    A = rng.standard_normal((L, rank))
    return A @ A.T


def test_curve_samples_factor_reproduces_the_block():
    import causalgpslc_jl_amd as gp
    rng = np.random.default_rng(41)
    S, L, G = 3, 6, 2
    cov = np.zeros((S, L, L, G))
    for s in range(S):
        for g in range(G):
            cov[s, :, :, g] = _random_psd(rng, L, L) * 10.0 ** (g - s)
    F = _factor(gp, cov)
    for s in range(S):
        for g in range(G):
            Cb, Fb = cov[s, :, :, g], F[:, :, s, g]
            assert np.max(np.abs(Fb @ Fb.T - Cb)) <= 4 * L * L * EPS * np.max(np.diag(Cb)), (s, g)
            assert np.allclose(Fb, cu.pivoted_factor(Cb), rtol=1e-10, atol=1e-12 * np.sqrt(np.max(np.diag(Cb))))


def test_curve_samples_rank_deficient_block():
    """Two equal levels and no jitter: a singular block is a normal input; the factor has one zero column."""
    import causalgpslc_jl_amd as gp
    c = cases.make_case(40, "UX", False, S=2, seed=43)
    w = np.full((1, 40), 1 / 40)
    lv = np.array([0.6, -0.3, 0.6, 0.1])
    exp = cu.expected_curve(c, lv, w, pred_noise=0.0)
    cov = exp["cov"]
    cov[:, 2, :, :] = cov[:, 0, :, :]            # the repeated level, bit for bit
    cov[:, :, 2, :] = cov[:, :, 0, :]
    F = _factor(gp, cov)
    for s in range(2):
        Cb, Fb = cov[s, :, :, 0], F[:, :, s, 0]
        assert np.max(np.abs(Fb @ Fb.T - Cb)) <= 4 * 16 * EPS * np.max(np.diag(Cb))
        assert np.all(Fb[:, 3] == 0.0) and np.any(Fb[:, 2] != 0.0)
        assert np.array_equal(Fb[0], Fb[2])      # the two equal levels move together in every draw


def test_curve_samples_slightly_indefinite_block():
    import causalgpslc_jl_amd as gp
    rng = np.random.default_rng(44)
    L = 5
    Q, _ = np.linalg.qr(rng.standard_normal((L, L)))
    Cb = (Q * np.array([2.0, 1.0, 0.3, 1e-3, -2e-16])) @ Q.T
    Cb = 0.5 * (Cb + Cb.T)
    Fb = _factor(gp, Cb[None, :, :, None])[:, :, 0, 0]
    assert np.all(np.isfinite(Fb))
    assert np.max(np.abs(Fb @ Fb.T - Cb)) <= 4 * L * L * EPS * np.max(np.diag(Cb))
    assert np.all(Fb[:, 4] == 0.0)
    # an all-zero block (a zero weight column) and a negative one: no factor at all, the draws are the mean
    out = gp.curveSamples(np.full((1, L, 1), 3.0), np.zeros((1, L, L, 1)), 2, seed=1)
    assert np.all(out == 3.0)
    out = gp.curveSamples(np.full((1, L, 1), 3.0), -np.eye(L)[None, :, :, None], 2, seed=1)
    assert np.all(out == 3.0)


def test_curve_samples_single_level_layout_and_philox():
    import causalgpslc_jl_amd as gp
    rng = np.random.default_rng(45)
    # L = 1: mean + sqrt(var) z (a covariance, unlike gpslc_sate_samples' use of the variance as sigma)
    m1, v1 = rng.standard_normal((4, 1, 2)), rng.random((4, 1, 1, 2)) + 0.1
    z1 = rng.standard_normal((1, 3, 4, 2))
    got = gp.curveSamples(m1, v1, 3, z=z1)
    assert np.allclose(got[0], m1[:, 0, :][None, :, :] + np.sqrt(v1[:, 0, 0, :])[None, :, :] * z1[0], rtol=1e-14, atol=1e-15)
    # layout of out and z against the NumPy reference, distinct blocks per (s, g)
    S, L, G, spp = 3, 4, 2, 5
    mean = rng.standard_normal((S, L, G))
    cov = np.zeros((S, L, L, G))
    for s in range(S):
        for g in range(G):
            cov[s, :, :, g] = _random_psd(rng, L, L if (s + g) % 2 else 2)
    z = rng.standard_normal((L, spp, S, G))
    got = gp.curveSamples(mean, cov, spp, z=z)
    ref = cu.curve_samples(mean, cov, spp, z)
    assert got.shape == (L, spp, S, G)
    assert np.allclose(got, ref, rtol=1e-10, atol=1e-10)
    # the Philox stream: reproducible, seed-dependent, stream id 2^41 + s + S g, element k + L d, standard normal moments
    a, b, d = gp.curveSamples(mean, cov, spp, seed=7), gp.curveSamples(mean, cov, spp, seed=7), gp.curveSamples(mean, cov, spp, seed=8)
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    for s, g in ((0, 0), (2, 1)):
        zz = orc.philox_normals(7, (1 << 41) + s + S * g, L * spp).reshape(L, spp, order="F")
        assert np.allclose(a[:, :, s, g], mean[s, :, g][:, None] + cu.pivoted_factor(cov[s, :, :, g]) @ zz, rtol=1e-10, atol=1e-10)
    big = gp.curveSamples(np.zeros((1, 2, 1)), np.eye(2)[None, :, :, None], 20000, seed=3)[:, :, 0, 0]
    assert abs(big.mean()) < 0.03 and abs(big.var() - 1.0) < 0.03 and abs(np.corrcoef(big)[0, 1]) < 0.03


def test_curve_samples_argument_errors():
    from causalgpslc_jl_amd import _lib
    lib = _lib.load()
    m, cv, out = np.zeros((2, 3, 1)), np.zeros((2, 3, 3, 1)), np.full((3, 2, 2, 1), 7.0)

    def call(mean=m, cov=cv, S=2, L=3, G=1, spp=2, o=out):
        return lib.gpslc_curve_samples(_p(mean), _p(cov), S, L, G, spp, 0, None, _p(o))

    assert call(mean=None) == -1 and call(cov=None) == -2 and call(S=-1) == -3
    assert call(L=0) == -4 and call(G=0) == -5 and call(spp=-1) == -6 and call(o=None) == -9
    assert np.all(out == 7.0)
    assert call(S=0) == 0 and call(spp=0) == 0 and np.all(out == 7.0)
    assert call() == 0 and np.all(out == 0.0)


# ---- the Python mirror: parsing and refusals, before any device call -------------------------------------------------
def test_effect_curve_signatures():
    import causalgpslc_jl_amd as gp
    par = inspect.signature(gp.effectCurve).parameters
    assert list(par)[:4] == ["g", "doTs", "baseline", "weights"] and par["weights"].default is None
    par = inspect.signature(gp.sampleEffectCurve).parameters
    assert list(par)[:7] == ["g", "doTs", "samplesPerPosterior", "z", "seed", "baseline", "weights"]
    assert par["samplesPerPosterior"].default == 10 and par["seed"].default == 0


def test_effect_curve_refusals_come_before_any_device_call():
    import causalgpslc_jl_amd as gp
    c = cases.make_case(12, "UX", False, S=2, seed=1)
    g = cases.gpslc_object(gp, c)
    n = c["n"]
    D = np.stack([c["T"] + 0.5, c["T"]])
    for fn in (gp.effectCurve, gp.sampleEffectCurve):
        with pytest.raises(ValueError, match="scalar levels"):
            fn(g, D)                                               # vector levels
        with pytest.raises(NotImplementedError, match="devices"):
            fn(g, [0.6, 0.2], devices=[0, 0])
        with pytest.raises(ValueError, match=f"n = {n}"):
            fn(g, [0.6], weights=np.ones(n + 1))
        with pytest.raises(ValueError, match="empty group mask"):
            fn(g, [0.6], weights=np.zeros(n, dtype=bool))
        with pytest.raises(ValueError, match="non-finite"):
            fn(g, [0.6], weights=np.full(n, np.nan))
        with pytest.raises(ValueError, match="L = 2"):
            fn(g, [0.6, 0.1], baseline=[0.0, 0.1, 0.2])
    assert g._ctx is None                                          # nothing above reached the device


def test_header_declares_the_curve_symbols_and_the_binding_table_has_them():
    from causalgpslc_jl_amd import _lib
    syms = set(_lib.header_symbols())
    for name in ("gpslc_predict_curve", "gpslc_curve_samples"):
        assert name in syms and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    # covW more than gpslc_predict_weighted
    assert len(_lib.SIGNATURES["gpslc_predict_curve"][1]) == len(_lib.SIGNATURES["gpslc_predict_weighted"][1]) + 1
    txt = open(_lib.HEADER_PATH).read()
    assert "s + S*(l + L*(l' + L*g))" in txt and "out[l + L*(d + spp*(s + S*g))]" in txt
