"""Predictions for new individuals on the GPU over the feature width F = nU + nX (gpslc_predict_new).
tests/test_gpu_new_individuals.py runs every case at nU = 2, nX = 3; here the cases of tests/new_individuals_widths.py —
lengthscales normalised so that the kernel stays of order one at every width, which tests/test_new_individuals_widths.py pins on
the CPU together with the sensitivity of every case to one dropped feature (>= 1e6 x the tight bound).

Kernels launched, (F, form) per test — new_mean_mfma_kernel<FREG, FORM> has FREG = 4 (F <= 4), 6, 8, 10, 12 and 0 (F >= 13):
  test_widths_against_restatement         F = 1, 1, 4 | 6 | 7, 8 | 9, 10 | 11, 12 | 13, 13, 13, 32, 32, 32, 32, each x 3 forms: all 18
                                          instantiations, and new_build_kernel<FORM> at F = 32 (66,816 bytes of LDS: its opt-in)
  test_constant_columns_move_no_bit       F = 5 (rung 6) against F = 6, 7, 9, 11, 13, 32 x 3 forms x 3 placements
  test_copies_reproduce_the_training_side F = 4, 6, 8, 10, 12, 13, 32 x 3 forms against ite_mean_mfma_kernel (L = 5 > 4)
  test_the_unew_sample_stride             F = 13 (nU = 5), S = 3 in chunks of one sample

Bounds: test_gpu_new_individuals._check_new (test_gpu_contrast._check's 1e-6, then 1e-9), imported; everything else is bit for bit
(offscale.bits_equal).  No bound of this file is its own."""
import functools

import numpy as np
import pytest

import cases
import new_individuals_restatement as nr
import new_individuals_widths as nw
from offscale import bits_differ, bits_equal
from test_gpu_new_individuals import _call, _check_new, _cov_slnn

pytestmark = pytest.mark.gpu
ROWS = [0, 5, 127, 128, 64]          # both training tiles, the tile's last row and the second tile's only live row


def _same(name, a, b):
    assert bits_equal(a, b), f"{name}: {bits_differ(a, b)}"


@functools.lru_cache(maxsize=None)
def _object(gp, nU, nX):
    return cases.gpslc_object(gp, nw.width_case(nU, nX))


# ---- 1. every width against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("nU,nX", nw.WIDTHS)
def test_widths_against_restatement(gp, nU, nX, form):
    c, g = nw.width_case(nU, nX), _object(gp, nU, nX)
    Xn, Un = nw.width_new(nU, nX)
    lv, doT, base = nw.levels(form)
    st, mean, var, cov = _call(g, nw.M, Xn, Un, form, doT, base)
    assert st == 0 and (Xn is None) == (nX == 0) and (Un is None) == (nU == 0)
    assert mean.shape == var.shape == (nw.M, nw.S, nw.L) and cov.shape == (nw.M, nw.M, nw.S, nw.L)
    _check_new(nr.expected(c, Xn, Un, nw.M, form, lv), mean, var, _cov_slnn(cov), c)


def test_one_feature_more_than_the_kernels_hold_is_refused(gp):
    """MAXF = 32 features is what the kernels' LDS layouts hold: gpslc_create refuses nX + nU = 33 with -4 and takes 32"""
    for nX, nU in ((33, 0), (0, 33), (20, 13)):
        with pytest.raises(gp.GPSLCError) as ei:
            gp.Context(10, nX, nU)
        assert ei.value.status == -4
    gp.Context(10, 20, 12).close()


# ---- 2. constant columns move no bit ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unpadded(gp, form):
    lv, doT, base = nw.levels(form)
    out = _call(_object(gp, 2, 3), nw.M, *nw.width_new(2, 3), form, doT, base)
    assert out[0] == 0
    _check_new(nr.expected(nw.width_case(2, 3), *nw.width_new(2, 3), nw.M, form, lv), out[1], out[2], _cov_slnn(out[3]),
               nw.width_case(2, 3))
    return out


@pytest.mark.parametrize("k", nw.PAD_COUNTS)
@pytest.mark.parametrize("place", nw.PAD_PLACES)
def test_constant_columns_move_no_bit(gp, place, k):
    """k constant columns beside the five real ones (behind X, in front of X, behind U; a nonzero value and a lengthscale of
    its own per column): x (1 / l) is the same product on both sides of every pair, the difference is 0.0 and
    fma(0.0, 0.0, lux) = lux with lux >= +0 — in the mean kernel whichever rung serves the wider F, in the tile builder and in
    the Gram build behind the factor.  So mean, var and cov are the unpadded call's, bit for bit: pair_mfma.h's "which rung
    serves an F cannot change a bit", from outside."""
    c = nw.width_case(2, 3)
    cp, Xp, Up = nw.pad_constant(c, *nw.width_new(2, 3), k, place)
    g = cases.gpslc_object(gp, cp)
    assert g.getNU() + g.getNX() == 5 + k
    for form in nr.FORMS:
        _, doT, base = nw.levels(form)
        st, mean, var, cov = _call(g, nw.M, Xp, Up, form, doT, base)
        ref = _unpadded(gp, form)
        assert st == 0 and np.all(np.isfinite(ref[1])) and np.any(ref[1] != 0.0)
        for name, a, b in zip(("mean", "var", "cov"), (mean, var, cov), ref[1:]):
            _same(f"{place} k={k} {form} {name}", a, b)
    g.ctx().close()


# ---- 3. copies reproduce the training-side kernels ------------------------------------------------------------------------
def _train_kw(form, base):
    return dict(outcome=True) if form == "outcome" else dict(baseline=base) if form == "contrast" else dict(slope=True)


@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("nU,nX", nw.ONE_PER_RUNG)
def test_copies_reproduce_the_training_side(gp, nU, nX, form):
    """New individuals that copy training rows, five levels (from L = 5 `predict` takes ite_mean_mfma_kernel): the mean is that
    kernel's MeanITE of the row, bit for bit (the same staged R, the same pair-product body, the same row of
    B); var and cov against ITEDistributions at level 0 within _check_new's bounds (another route: the n x n tiles)."""
    c, g = nw.width_case(nU, nX), _object(gp, nU, nX)
    Xn, Un = nr.new_individuals(c, len(ROWS), seed=2, copies=list(enumerate(ROWS)))
    lv, doT, base = nw.levels(form, 5)
    st, mean, var, cov = _call(g, len(ROWS), Xn, Un, form, doT, base)
    assert st == 0
    mi = gp.predict(g, doT, want_mean_ite=True, **_train_kw(form, base))[2]
    assert mi.shape == (nw.N, nw.S, 5) and np.all(np.isfinite(mi)) and np.any(mi != 0.0)
    _same(f"nU={nU} nX={nX} {form}: mean against MeanITE", mean, mi[ROWS])
    M, Cv = gp.ITEDistributions(g, doT[0], **_train_kw(form, None if base is None else base[0]))
    exp = dict(mean=M[:, ROWS].T[:, :, None], var=np.stack([np.diag(Cv[s])[ROWS] for s in range(nw.S)], axis=1)[:, :, None],
               cov=np.stack([Cv[s][np.ix_(ROWS, ROWS)] for s in range(nw.S)])[:, None])
    _check_new(exp, mean[:, :, :1], var[:, :, :1], _cov_slnn(cov)[:, :1], c)


def test_like_copies_the_latent_confounders(gp):
    """the front end's like=: U[like[i], :, s] for every sample — the call above through predictNew"""
    nU, nX = 5, 8
    c, g = nw.width_case(nU, nX), _object(gp, nU, nX)
    lv, doT, base = nw.levels("contrast", 5)
    mean, var, cov = gp.predictNew(g, doT, Xnew=c["X"][ROWS], like=ROWS, baseline=base, want_cov=True)
    Xn, Un = nr.new_individuals(c, len(ROWS), seed=2, copies=list(enumerate(ROWS)))
    st, mean2, var2, cov2 = _call(g, len(ROWS), Xn, Un, "contrast", doT, base)
    assert st == 0
    _same("mean", mean, mean2)
    _same("var", var, var2)
    _same("cov", cov, _cov_slnn(cov2))
    _same("mean against MeanITE", mean, gp.predict(g, doT, want_mean_ite=True, baseline=base)[2][ROWS])


# ---- 4. the sample stride of Unew ------------------------------------------------------------------------------------------
def test_the_unew_sample_stride(gp):
    """Unew is m x nU x S with sample stride m nU, read as Unew + s m nU by a chunk that starts at sample s0 > 0 (max_batch = 1:
    one sample per chunk).  nU = 5, m = 130, S = 3: the first five new individuals copy training rows in X and in SAMPLE 1's
    block of Unew only.  Their means of sample 1 are those rows' MeanITE bits; of samples 0 and 2 they are not; and all of it
    agrees with the restatement."""
    nU, nX, S = 5, 8, 3
    c = nw.width_case(nU, nX, S=S)
    Xn, Un = nr.new_individuals(c, nw.M, seed=3)
    k = len(ROWS)
    Xn[:k] = c["X"][ROWS]
    Un[:k, :, 1] = c["U"][ROWS, :, 1]
    lv, doT, base = nw.levels("outcome", 5)
    g = cases.gpslc_object(gp, c)
    whole = _call(g, nw.M, Xn, Un, "outcome", doT, base)
    mi = gp.predict(g, doT, want_mean_ite=True, outcome=True)[2]
    g1 = cases.gpslc_object(gp, c)
    g1.ctx().set_tuning(max_batch=1)
    chunked = _call(g1, nw.M, Xn, Un, "outcome", doT, base)
    assert whole[0] == 0 and chunked[0] == 0
    for name, a, b in zip(("mean", "var", "cov"), chunked[1:], whole[1:]):
        _same(name + ": one sample per chunk against one chunk", a, b)
    mean = chunked[1]
    _same("sample 1 against MeanITE", mean[:k, 1], mi[ROWS, 1])
    for s in (0, 2):
        assert not np.any(mean[:k, s] == mi[ROWS, s]), s
    _check_new(nr.expected(c, Xn, Un, nw.M, "outcome", lv), mean, chunked[2], _cov_slnn(chunked[3]), c)
    g.ctx().close()
    g1.ctx().close()
