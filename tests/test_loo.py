"""Leave-one-out predictive checks, host side: the restatement's two computations agree, looSummary's arithmetic, and the new
symbol in the binding table and in the built library."""
import ctypes
import math
import os

import numpy as np
import pytest

import cases
import loo_restatement as lr


@pytest.mark.parametrize("binary_t", [False, True])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
@pytest.mark.parametrize("n", [1, 3, 24, 129, 200, 300, 400])
def test_closed_form_equals_the_literal_refit(n, shape, binary_t):
    """diag(inv(A)) / inv(A) Y against deleting row and column i and conditioning on the rest, within the GPU tests' bound
    max(1e-10, 1e-14 cond(A)) — on these well-conditioned cases its floor, 1e-10 (the two differ by a few 1e-14)."""
    c = cases.make_case(n, shape, binary_t, S=1, seed=7 + n)
    e = lr.expected(c)[0]
    assert e["cond"] <= 1e4 and e["tol"] == 1e-10
    errs = lr.errors(e["closed"], e["refit"], c["Y"])
    print(n, shape, binary_t, "cond", e["cond"], "errors (var, mean, lpd)", errs)
    assert max(errs) <= e["tol"], errs


def test_refit_is_the_textbook_conditional_on_a_hand_made_matrix():
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    Y = np.array([1.0, -1.0])
    mean, var, lpd = lr.refit(A, Y)
    assert np.allclose(mean, [0.5 * -1.0 / 1.0, 0.5 * 1.0 / 2.0], rtol=1e-15)
    assert np.allclose(var, [2.0 - 0.25 / 1.0, 1.0 - 0.25 / 2.0], rtol=1e-15)
    assert np.allclose(lpd, [-0.5 * math.log(2 * math.pi * v) - 0.5 * (y - m) ** 2 / v for y, m, v in zip(Y, mean, var)])
    for a, b in zip(lr.closed_form(A, Y), (mean, var, lpd)):
        assert np.allclose(a, b, rtol=1e-14)


def test_loo_summary_arithmetic_on_hand_made_arrays():
    import causalgpslc_jl_amd as gp
    Y = np.array([1.0, 0.0, -2.0])
    g = gp.GPSLCObject(None, np.zeros(3), Y, None, None, None, np.ones(2), np.ones(2), np.ones(2))
    mean = np.array([[0.0, 1.0], [0.0, 0.0], [0.0, -2.0]])
    var = np.array([[1.0, 4.0], [4.0, 1.0], [1.0, 0.25]])
    lpd = np.log(np.array([[0.1, 0.3], [0.2, 0.2], [1e-300, 0.5]]))
    s = gp.looSummary(g, loo=(mean, var, lpd))
    assert np.allclose(s["elpd"], [math.log(0.1 * 0.2 * 1e-300), math.log(0.3 * 0.2 * 0.5)], rtol=1e-15)
    assert np.allclose(s["pointwise"], np.log([0.2, 0.2, 0.25]), rtol=1e-14)
    z = np.array([[1.0, 0.0], [0.0, 0.0], [-2.0, 0.0]])
    assert np.array_equal(s["zscore"], z)
    phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    assert np.allclose(s["pit"], [(phi(1.0) + 0.5) / 2, 0.5, (phi(-2.0) + 0.5) / 2], rtol=1e-15)
    # an override is the outcome vector the z-scores are taken of
    s2 = gp.looSummary(g, Y_override=Y + 1.0, loo=(mean, var, lpd))
    assert np.array_equal(s2["zscore"], (Y[:, None] + 1.0 - mean) / np.sqrt(var))
    # log-mean-exp survives densities far below the smallest double
    far = gp.looSummary(g, loo=(mean, var, np.full((3, 2), -5000.0)))
    assert np.allclose(far["pointwise"], -5000.0) and np.allclose(far["elpd"], -15000.0)


def test_symbol_is_in_the_binding_table():
    from causalgpslc_jl_amd import _lib
    res, args = _lib.SIGNATURES["gpslc_y_loo"]
    assert res is ctypes.c_int and len(args) == 14 and args[1] is ctypes.c_int64
    assert "gpslc_y_loo" in _lib.header_symbols()
    import causalgpslc_jl_amd as gp
    assert callable(gp.looPredictive) and callable(gp.looSummary) and hasattr(gp.Context, "y_loo")


def test_built_library_exports_the_symbol():
    from causalgpslc_jl_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    # the symbol table of the file itself: loading the library is not needed (and needs the HIP runtime)
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"\0gpslc_y_loo\0" in data and b"\0gpslc_y_logpdf\0" in data
