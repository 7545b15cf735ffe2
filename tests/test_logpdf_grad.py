"""The host restatement of the gradient of the outcome log-likelihood (grad_restatement.py) checked on itself: no GPU.

1. fp64 against long double: within 1e-3 of the bound tol * scale the GPU tests use — the restatement's own rounding is no part
   of the bound's budget.  Measured: 8.8e-4 of the bound for dY (n = 200), 5.0e-4 for dyNoise (cond 1.8e6), at most 1.2e-5 for dU
   and the lengthscales.
2. The long-double closed form against central differences (h = 1e-6) of a long-double log density, to 1e-9 of the scale.
3. The inputs of the GPU tests can see two mistakes of a tiled implementation at n = 129 (one live row in the second tile):
   without the column sums of the off-diagonal tile dU moves by more than 1e6 bounds.  Letting the padding take part cannot move
   dU or the lengthscale gradients at all — on the padding alpha and the off-diagonal of A^-1 are exact zeros and the diagonal
   meets D_ii = 0, so every extra term is an exact zero, which the test asserts — but it adds the padded diagonal of A^-1 to
   sum c: dyNoise and dyScale move by more than 1e6 bounds."""
import numpy as np
import pytest

import grad_restatement as gr


@pytest.mark.parametrize("k", range(len(gr.RANDOM_CASES)))
def test_fp64_restatement_lies_well_inside_the_bound(k):
    W, ls, ys, yn, Y, nU, nX = gr.random_inputs()[k]
    n = len(Y)
    tol, cond = gr.tolerance(W, ls, ys, yn)
    g64, _ = gr.gradient(W, ls, ys, yn, Y, nU, nX, np.float64)
    gl, sl = gr.gradient(W, ls, ys, yn, Y, nU, nX, np.longdouble)
    err = gr.errors(g64, gl, sl)
    print("n", n, "cond %.3g tol %.3g" % (cond, tol), "fp64 error / bound:", {k: v / tol for k, v in err.items()})
    assert max(err.values()) <= 1e-3 * tol, err


@pytest.mark.parametrize("n,nU,nX", [(24, 2, 3), (60, 1, 0)])
def test_closed_form_matches_central_differences(n, nU, nX):
    W, ls, ys, yn, Y, nU, nX = gr.random_inputs(2, ((n, nU, nX, 0.2, (1.5, 3.0)),))[0]
    F = nU + nX + 1
    g, sc = gr.gradient(W, ls, ys, yn, Y, nU, nX, np.longdouble)
    h = np.longdouble(1e-6)
    ld = np.longdouble

    def fd(f):
        return (f(h) - f(-h)) / (2 * h)

    eye = np.eye(F, dtype=ld)
    dls = np.concatenate([g["duyLS"], g["dxyLS"], [g["dtyLS"]]])
    sls = np.concatenate([sc["duyLS"], sc["dxyLS"], [sc["dtyLS"]]])
    for f in range(F):
        num = fd(lambda e: gr.logpdf(W.astype(ld), ls.astype(ld) + e * eye[f], ys, yn, Y))
        assert abs(num - dls[f]) <= 1e-9 * sls[f], ("lengthscale", f, num, dls[f])
    for i in range(0, n, 7):
        for f in range(nU):
            def moved(e):
                W2 = W.astype(ld)
                W2[i, f] += e
                return gr.logpdf(W2, ls, ys, yn, Y)
            num = fd(moved)
            assert abs(num - g["dU"][i, f]) <= 1e-9 * sc["dU"][i, f], ("U", i, f, num, g["dU"][i, f])
    num = fd(lambda e: gr.logpdf(W, ls, ld(ys) + e, yn, Y))
    assert abs(num - g["dyScale"]) <= 1e-9 * sc["dyScale"], ("yScale", num, g["dyScale"])
    num = fd(lambda e: gr.logpdf(W, ls, ys, ld(yn) + e, Y))
    assert abs(num - g["dyNoise"]) <= 1e-9 * sc["dyNoise"], ("yNoise", num, g["dyNoise"])
    for i in (3, n - 1):
        num = fd(lambda e: gr.logpdf(W, ls, ys, yn, Y.astype(ld) + e * np.eye(n, dtype=ld)[i]))
        assert abs(num - g["dY"][i]) <= 1e-9 * sc["dY"][i], ("Y", i, num, g["dY"][i])


def test_the_inputs_can_see_a_missing_column_sum_and_an_unmasked_padding():
    W, ls, ys, yn, Y, nU, nX = gr.random_inputs()[0]
    tol, _ = gr.tolerance(W, ls, ys, yn)
    good, sc = gr.gradient(W, ls, ys, yn, Y, nU, nX)
    move = gr.errors(gr.gradient(W, ls, ys, yn, Y, nU, nX, no_colsum=True)[0], good, sc)
    print("without the column sums, in bounds:", {k: v / tol for k, v in move.items()})
    assert move["dU"] > 1e6 * tol
    pad, _ = gr.gradient(W, ls, ys, yn, Y, nU, nX, no_mask=True)
    move = gr.errors(pad, good, sc)
    print("with the padding taking part, in bounds:", {k: v / tol for k, v in move.items()})
    assert move["dyNoise"] > 1e6 * tol and move["dyScale"] > 1e6 * tol
    # every extra term of the pair sums is an exact zero; the sums themselves are re-associated by the 127 extra zeros
    assert max(move["dU"], move["duyLS"], move["dxyLS"], move["dtyLS"]) <= 1e-3 * tol


def test_shift_identity_of_the_restatement():
    """the likelihood does not change when a column of U is shifted: sum_i dU[i, f] vanishes to the bound"""
    W, ls, ys, yn, Y, nU, nX = gr.random_inputs()[0]
    tol, _ = gr.tolerance(W, ls, ys, yn)
    g, sc = gr.gradient(W, ls, ys, yn, Y, nU, nX)
    assert np.all(np.abs(g["dU"].sum(0)) <= tol * sc["dU"].sum(0))
