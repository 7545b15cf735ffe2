"""Leave-group-out predictive checks, host side: the restatement's two computations agree, lgoSummary's and foldLabels'
arithmetic, label compaction, and the new symbol in the binding table and in the built library."""
import ctypes
import math
import os

import numpy as np
import pytest

import cases
import lgo_restatement as lg


def _labellings(n):
    out = {"mod7": lg.mod7(n), "blocks17": lg.blocks_of(n, 17)}
    if n <= 128:
        out["one group"] = lg.one_group(n)
    if n <= 129:
        out["singletons"] = lg.singletons(n)
    if n >= 136:
        out["rows 120..135"] = lg.with_block(n, 120, 136)
    if n >= 400:
        out["rows 100..227"] = lg.with_block(n, 100, 228)
    return out


@pytest.mark.parametrize("shape", list(cases.SHAPES))
@pytest.mark.parametrize("n", [3, 24, 128, 129, 200, 400])
def test_closed_form_equals_the_literal_refit(n, shape):
    """inv(A)[I, I] through its Cholesky factor against deleting the group and conditioning on the rest, within the GPU tests'
    bound max(1e-10, 1e-14 cond(A) max_g cond(C_g)) (on these cases mostly its floor; the two differ by a few 1e-15)"""
    c = cases.make_case(n, shape, False, S=1, seed=7 + n)
    for name, labels in _labellings(n).items():
        e = lg.expected(c, labels)[0]
        errs = lg.errors(e["closed"], e["refit"], e["q"], c["Y"], labels)
        print(n, shape, name, "cond(A) %.3g cond(C) %.3g tol %.3g" % (e["cond"], e["cond_c"], e["tol"]), "errors (var, mean, lpd)", errs)
        assert max(errs) <= e["tol"], (name, errs)


def test_refit_is_the_textbook_conditional_on_a_hand_made_matrix():
    """3 x 3, the group {0, 1} predicted from individual 2 and individual 2 from the group"""
    A = np.array([[2.0, 0.5, 0.3], [0.5, 1.0, 0.2], [0.3, 0.2, 1.5]])
    Y = np.array([1.0, -1.0, 0.5])
    labels = np.array([0, 0, 1], dtype=np.int32)
    (mean, var, lpd), q = lg.refit(A, Y, labels)
    k = A[:2, 2]
    mu = k * Y[2] / A[2, 2]
    cov = A[:2, :2] - np.outer(k, k) / A[2, 2]
    r = Y[:2] - mu
    q0 = r @ np.linalg.solve(cov, r)
    assert np.allclose(mean[:2], mu, rtol=1e-14) and np.allclose(var[:2], np.diag(cov), rtol=1e-14)
    assert math.isclose(q[0], q0, rel_tol=1e-13)
    assert math.isclose(lpd[0], -math.log(2 * math.pi) - 0.5 * math.log(np.linalg.det(cov)) - 0.5 * q0, rel_tol=1e-13)
    sol = np.linalg.solve(A[:2, :2], np.column_stack([Y[:2], k]))
    m2, v2 = k @ sol[:, 0], A[2, 2] - k @ sol[:, 1]
    assert math.isclose(mean[2], m2, rel_tol=1e-13) and math.isclose(var[2], v2, rel_tol=1e-13)
    assert math.isclose(lpd[1], -0.5 * math.log(2 * math.pi * v2) - 0.5 * (Y[2] - m2) ** 2 / v2, rel_tol=1e-13)
    (cm, cv, cl), conds = lg.closed_form(A, Y, labels)
    assert np.allclose(cm, mean, rtol=1e-13) and np.allclose(cv, var, rtol=1e-13) and np.allclose(cl, lpd, rtol=1e-13)
    # the label number does not matter
    (pm, pv, pl), _ = lg.refit(A, Y, 1 - labels)
    assert np.array_equal(pm, mean) and np.array_equal(pv, var) and np.array_equal(pl, lpd[::-1])


def _object(gp, Y, obj=None):
    g = gp.GPSLCObject(None, np.zeros(len(Y)), Y, None, None, None, np.ones(2), np.ones(2), np.ones(2))
    if obj is not None:
        g.obj = obj
    return g


def test_lgo_summary_arithmetic_on_hand_made_arrays():
    import causalgpslc_jl_amd as gp
    Y = np.array([1.0, 0.0, -2.0])
    g = _object(gp, Y)
    mean = np.array([[0.0, 1.0], [0.0, 0.0], [0.0, -2.0]])
    var = np.array([[1.0, 4.0], [4.0, 1.0], [1.0, 0.25]])
    lpd = np.log(np.array([[0.1, 0.3], [1e-300, 0.5]]))          # two groups
    keys = np.array(["a", "b"])
    s = gp.lgoSummary(g, lgo=(mean, var, lpd, keys))
    assert np.allclose(s["elpd"], [math.log(0.1 * 1e-300), math.log(0.3 * 0.5)], rtol=1e-15)
    assert np.allclose(s["groupwise"], np.log([0.2, 0.25]), rtol=1e-14)
    assert np.array_equal(s["zscore"], np.array([[1.0, 0.0], [0.0, 0.0], [-2.0, 0.0]]))
    phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))           # noqa: E731
    assert np.allclose(s["pit"], [(phi(1.0) + 0.5) / 2, 0.5, (phi(-2.0) + 0.5) / 2], rtol=1e-15)
    assert list(s["keys"]) == ["a", "b"]
    s2 = gp.lgoSummary(g, Y_override=Y + 1.0, lgo=(mean, var, lpd, keys))
    assert np.array_equal(s2["zscore"], (Y[:, None] + 1.0 - mean) / np.sqrt(var))
    far = gp.lgoSummary(g, lgo=(mean, var, np.full((2, 2), -5000.0), keys))
    assert np.allclose(far["groupwise"], -5000.0) and np.allclose(far["elpd"], -10000.0)


@pytest.mark.parametrize("n,K", [(10, 3), (7, 7), (128, 5), (5, 1)])
def test_fold_labels(n, K):
    import causalgpslc_jl_amd as gp
    lab = gp.foldLabels(n, K, seed=3)
    assert lab.shape == (n,) and lab.dtype == np.int32
    sizes = np.bincount(lab, minlength=K)
    assert len(sizes) == K and sizes.sum() == n and sizes.max() - sizes.min() <= 1 and sizes.min() >= 1
    assert np.array_equal(lab, gp.foldLabels(n, K, seed=3))
    if 1 < K < n and n > 10:
        assert not np.array_equal(lab, gp.foldLabels(n, K, seed=4))
        assert not np.array_equal(lab, np.arange(n) % K)                 # shuffled, not dealt in row order
    for bad in (0, n + 1):
        with pytest.raises(ValueError):
            gp.foldLabels(n, bad, seed=0)


def test_label_compaction_with_string_keys_and_the_obj_column():
    from causalgpslc_jl_amd import api
    import causalgpslc_jl_amd as gp
    Y = np.zeros(5)
    keys, lab = api._group_labels(_object(gp, Y), ["s2", "s1", "s2", "s10", "s1"])
    assert list(keys) == ["s1", "s10", "s2"] and list(lab) == [2, 0, 2, 1, 0] and lab.dtype == np.int32
    keys, lab = api._group_labels(_object(gp, Y), np.array([40, 7, 7, 40, 9]))
    assert list(keys) == [7, 9, 40] and list(lab) == [2, 0, 0, 2, 1]
    keys, lab = api._group_labels(_object(gp, Y, obj=["b", "b", "a", "a", "c"]), None)        # groups=None: the obj column
    assert list(keys) == ["a", "b", "c"] and list(lab) == [1, 1, 0, 0, 2]
    with pytest.raises(ValueError, match="obj"):
        api._group_labels(_object(gp, Y), None)
    with pytest.raises(ValueError, match="one label per individual"):
        api._group_labels(_object(gp, Y), [0, 1, 2])


def test_symbol_is_in_the_binding_table():
    from causalgpslc_jl_amd import _lib
    res, args = _lib.SIGNATURES["gpslc_y_lgo"]
    assert res is ctypes.c_int and len(args) == 16 and args[1] is ctypes.c_int64
    assert args[10] is ctypes.c_int32 and args[11] is _lib.c_int32_p
    assert "gpslc_y_lgo" in _lib.header_symbols()
    import causalgpslc_jl_amd as gp
    assert callable(gp.lgoPredictive) and callable(gp.lgoSummary) and callable(gp.foldLabels) and hasattr(gp.Context, "y_lgo")


def test_built_library_exports_the_symbol():
    from causalgpslc_jl_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    # the symbol table of the file itself: loading the library is not needed (and needs the HIP runtime)
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"\0gpslc_y_lgo\0" in data and b"\0gpslc_y_loo\0" in data
