"""Weighted average effects over groups, without a GPU: the structured formulas the library evaluates against
the literal restatement (tests/weighted_restatement.py: w' M and w' (CovITE + pred_noise I) w from the dense oracle), the
`weights=` / `groupWeights` parsing of the Python mirror and its refusals (all raised before any device call), and the symbol
in the public header."""
import inspect

import numpy as np
import pytest

import cases
import contrast_restatement as cr
import weighted_restatement as wr

GRID8 = [(shape, bt) for shape in sorted(cases.SHAPES) for bt in (False, True)]


def _levels(c, con):
    if con:
        A, B = cr.pairs(c, 1)
        return float(A[0]), float(B[0])
    return float(c["doTs"][1]), None


# ---- the derivation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bt", GRID8)
@pytest.mark.parametrize("n", [24, 129, 200, 400])
@pytest.mark.parametrize("con", [False, True])
def test_structured_formulas_against_the_literal_restatement(n, shape, bt, con):
    """bw = B w, kw = K w, c = D' w, w' Delta w, v = L^-1 c: mean = v . z and var = (w' Delta w - v . v) + pred_noise w . w
    reproduce w' MeanITE and w' (CovITE + pred_noise I) w for the seven weight vectors, inside the tight bounds."""
    c = cases.make_case(n, shape, bt, S=2, seed=11 + n)
    a, b = _levels(c, con)
    W = wr.weight_set(c, seed=n)
    exp = wr.expected_weighted(c, [a], W, base=None if b is None else [b])
    worst_m = worst_v = 0.0
    for s in range(c["S"]):
        for g in range(W.shape[0]):
            m, v = wr.structured(c, s, a, W[g], base=b)
            rm, rv = exp["mean"][s, 0, g], exp["var"][s, 0, g]
            _, _, tm, tv = wr.bounds(rm, rv, W[g], c["yScale"][s])
            worst_m, worst_v = max(worst_m, abs(m - rm) / tm), max(worst_v, abs(v - rv) / tv)
            assert abs(m - rm) <= tm, (s, wr.WEIGHT_NAMES[g], m, rm)
            assert abs(v - rv) <= tv, (s, wr.WEIGHT_NAMES[g], v, rv)
    print(f"worst error / tight bound: mean {worst_m:.2e} var {worst_v:.2e}")


def test_uniform_weights_are_the_sate_and_a_unit_vector_is_one_individual():
    c = cases.make_case(60, "UX", False, S=2, seed=3)
    n = c["n"]
    ref = cases.oracle_expected(c)
    W = np.vstack([np.full(n, 1.0 / n), np.eye(n)[7]])
    exp = wr.expected_weighted(c, c["doTs"], W)
    assert np.allclose(exp["mean"][:, :, 0], ref["meanSATE"], rtol=1e-12, atol=0)
    assert np.allclose(exp["var"][:, :, 0], ref["varSATE"], rtol=1e-12, atol=0)
    assert np.array_equal(exp["mean"][:, :, 1], ref["meanITE"][7])
    assert np.allclose(exp["var"][:, :, 1], ref["covITE"][:, :, 7, 7], rtol=1e-14, atol=0)


def test_the_difference_of_two_groups_is_not_the_sum_of_their_variances():
    """Why a difference is a weight vector of its own: the two group effects are correlated."""
    c = cases.make_case(60, "UX", True, S=1, seed=5)
    W = wr.weight_set(c)
    v = wr.expected_weighted(c, [1.0], W, base=[0.0])["var"][0, 0]
    assert v[3] > 0.0 and abs(v[3] - (v[1] + v[2])) > 0.05 * v[3]


# ---- the Python mirror: parsing and refusals, before any device call -------------------------------------------------
def _object(gp, n=12, bt=False):
    c = cases.make_case(n, "UX", bt, S=2, seed=1)
    return cases.gpslc_object(gp, c), c


def test_weights_is_a_keyword_of_the_sate_entry_points():
    import causalgpslc_jl_amd as gp
    for fn in (gp.predict, gp.SATEDistributions, gp.sampleSATE):
        par = inspect.signature(fn).parameters
        assert "weights" in par and par["weights"].default is None, fn.__name__
    assert callable(gp.groupWeights)


def test_weights_parsing():
    from causalgpslc_jl_amd import api
    n = 6
    W, vec = api._weights(np.arange(n) / 10.0, n)
    assert vec and W.shape == (1, n) and W.dtype == np.float64 and W.flags.c_contiguous
    assert np.array_equal(W[0], np.arange(n) / 10.0)                       # float weights are used as given: no normalisation
    W, vec = api._weights([1, 0, 0, 2, 0, 0], n)
    assert vec and np.array_equal(W[0], [1.0, 0, 0, 2.0, 0, 0])            # integers are numbers, not masks
    mask = np.array([True, False, True, True, False, False])
    W, vec = api._weights(mask, n)
    assert vec and np.array_equal(W[0], mask / 3.0)                        # a Bool vector is a group: its average
    W, vec = api._weights(np.stack([mask, ~mask]), n)
    assert not vec and W.shape == (2, n) and np.array_equal(W, np.stack([mask / 3.0, ~mask / 3.0]))
    W, vec = api._weights(np.ones((1, n)), n)
    assert not vec and W.shape == (1, n)                                   # a (1, n) array keeps its group axis
    W, vec = api._weights([mask, np.full(n, 0.5)], n)                      # rows of a sequence are parsed one by one
    assert not vec and np.array_equal(W[0], mask / 3.0) and np.array_equal(W[1], np.full(n, 0.5))
    with pytest.raises(ValueError, match="empty group mask"):
        api._weights(np.zeros(n, dtype=bool), n)
    with pytest.raises(ValueError, match="empty group mask"):
        api._weights(np.stack([mask, np.zeros(n, dtype=bool)]), n)
    for bad in (np.ones(n + 1), np.ones((2, n + 1)), np.ones((n, 2)), np.ones((2, 2, n)), np.float64(1.0), []):
        with pytest.raises(ValueError, match="n = 6"):
            api._weights(bad, n)
    for bad in (np.array([0.1, np.nan, 0, 0, 0, 0]), np.array([np.inf, 0, 0, 0, 0, 0])):
        with pytest.raises(ValueError, match="non-finite"):
            api._weights(bad, n)


def test_group_weights():
    import causalgpslc_jl_amd as gp
    keys, W = gp.groupWeights(["b", "a", "b", "c", "a", "b"])
    assert list(keys) == ["a", "b", "c"] and W.shape == (3, 6)
    assert np.array_equal(W[0], [0, 0.5, 0, 0, 0.5, 0]) and np.array_equal(W[2], [0, 0, 0, 1.0, 0, 0])
    assert np.allclose(W[1], [1 / 3, 0, 1 / 3, 0, 0, 1 / 3], rtol=1e-16)
    assert np.allclose(W.sum(axis=1), 1.0, rtol=1e-15)
    cnt = np.array([2, 3, 1])
    assert np.allclose((cnt / 6.0) @ W, np.full(6, 1 / 6), rtol=1e-15)     # a partition: the group means average to the SATE
    keys, W = gp.groupWeights(np.array([3, 1, 3, 1]))
    assert list(keys) == [1, 3] and np.array_equal(W, [[0, 0.5, 0, 0.5], [0.5, 0, 0.5, 0]])
    keys, W = gp.groupWeights(np.array([True, False, True]))
    assert list(keys) == [False, True] and np.array_equal(W, [[0, 1.0, 0], [0.5, 0, 0.5]])
    for bad in ([], np.zeros((2, 3)), 1.0):
        with pytest.raises(ValueError, match="labels"):
            gp.groupWeights(bad)


def test_weights_refusals_come_before_any_device_call():
    import causalgpslc_jl_amd as gp
    g, c = _object(gp)
    n = c["n"]
    w = np.full(n, 1.0 / n)
    D = np.stack([c["T"] + 0.5, c["T"]])
    with pytest.raises(ValueError, match="scalar levels"):
        gp.predict(g, D, weights=w)                                # vector levels
    with pytest.raises(ValueError, match="scalar levels"):
        gp.SATEDistributions(g, c["T"] + 0.5, weights=w)
    with pytest.raises(ValueError, match="scalar levels"):
        gp.sampleSATE(g, c["T"] + 0.5, weights=w)
    with pytest.raises(NotImplementedError, match="devices"):
        gp.predict(g, [0.6, 0.2], weights=w, devices=[0, 0])
    with pytest.raises(ValueError, match=f"n = {n}"):
        gp.predict(g, [0.6], weights=np.ones(n + 1))
    with pytest.raises(ValueError, match=f"n = {n}"):
        gp.SATEDistributions(g, 0.6, weights=np.ones((n, 2)))
    with pytest.raises(ValueError, match="empty group mask"):
        gp.sampleSATE(g, 0.6, weights=np.zeros(n, dtype=bool))
    with pytest.raises(ValueError, match="non-finite"):
        gp.predict(g, [0.6], weights=np.full(n, np.nan))
    with pytest.raises(ValueError, match="L = 1"):
        gp.predict(g, [0.6], baseline=[0.0, 0.1], weights=w)       # the baseline is still checked
    assert g._ctx is None                                          # nothing above reached the device


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_header_declares_the_weighted_symbol_and_the_binding_table_has_it():
    from causalgpslc_jl_amd import _lib
    assert "gpslc_predict_weighted" in set(_lib.header_symbols()) and "gpslc_predict_weighted" in _lib.SIGNATURES
    # doT_base_or_null, G and weights more than gpslc_predict
    assert len(_lib.SIGNATURES["gpslc_predict_weighted"][1]) == len(_lib.SIGNATURES["gpslc_predict"][1]) + 3
    txt = open(_lib.HEADER_PATH).read()
    assert "weights[i + n*g]" in txt and "s + S*(l + L*g)" in txt and "doT_base_or_null" in txt
