"""The feature-width cases of tests/test_gpu_new_individuals_widths.py without a GPU: conditions on the reference alone that keep
every case able to tell a right kernel from a wrong one, whatever its seed becomes.

  - the median kernel value B*_ij / yScale lies in [0.2, 0.8] (without new_individuals_widths.normalise it is 1e-7 at F = 8 and
    1e-14 at F = 13: A is the identity and the variance carries no information);
  - the restatement's two sides agree within the tight bound of the GPU test (test_new_individuals._close);
  - deleting the last feature column moves mean, var and cov by at least 1e6 times that bound, for every width, form and sample:
    a kernel that reads one feature too few, or the wrong column, cannot pass;
  - the constant columns of the padding test leave the restatement where it was (within the tight bound: NumPy sums 32 squares
    in another order than 5), and the padded widths land on the rungs the GPU test claims."""
import numpy as np
import pytest

import new_individuals_restatement as nr
import new_individuals_widths as nw
from test_new_individuals import _close


def test_the_widths_cover_every_rung_at_both_edges():
    F = sorted({nU + nX for nU, nX in nw.WIDTHS})
    assert F == [1, 4, 6, 7, 8, 9, 10, 11, 12, 13, 32]
    assert {nw.freg_rung(f) for f in F} == {4, 6, 8, 10, 12, 0}
    for lo, hi in ((5, 6), (7, 8), (9, 10), (11, 12)):                    # both edges of a rung; rung 6 from the padding test
        assert nw.freg_rung(lo) == nw.freg_rung(hi) == hi
    assert [nw.freg_rung(5 + k) for k in nw.PAD_COUNTS] == [6, 8, 10, 12, 0, 0] and 5 + nw.PAD_COUNTS[-1] == 32
    assert sorted(nw.freg_rung(nU + nX) for nU, nX in nw.ONE_PER_RUNG) == [0, 0, 4, 6, 8, 10, 12]
    shapes = {nw.shape_of(nU, nX) for nU, nX in nw.WIDTHS}
    assert shapes == {"U", "X", "UX"}
    for nU, nX in nw.WIDTHS:
        c = nw.width_case(nU, nX)
        assert (0 if c["U"] is None else c["U"].shape[1], 0 if c["X"] is None else c["X"].shape[1]) == (nU, nX)
        assert c["n"] == 129 and c["S"] == 2


@pytest.mark.parametrize("nU,nX", nw.WIDTHS)
def test_lengthscales_are_normalised_and_the_kernel_is_of_order_one(nU, nX):
    c = nw.width_case(nU, nX)
    Xn, Un = nw.width_new(nU, nX)
    assert (Xn is None) == (nX == 0) and (Un is None) == (nU == 0)
    assert (Xn if Xn is not None else Un).shape[0] == nw.M
    tot = sum(np.sum(1.0 / c[k] ** 2, axis=0) for k in ("uyLS", "xyLS") if c[k] is not None)
    assert np.allclose(tot, 0.5, rtol=1e-14, atol=0)
    for s in range(c["S"]):
        med = nw.median_kernel(c, s, Xn, Un)
        A = nr.blocks(c, s, Xn, Un, nw.M)[0]
        print(f"nU={nU} nX={nX} s={s} median B*/yScale {med:.3f} cond(A) {np.linalg.cond(A):.3g}")
        assert 0.2 <= med <= 0.8, med


@pytest.mark.parametrize("form", nr.FORMS)
@pytest.mark.parametrize("nU,nX", nw.WIDTHS)
def test_literal_agrees_with_structured_and_a_dropped_feature_is_seen(nU, nX, form):
    c = nw.width_case(nU, nX)
    Xn, Un = nw.width_new(nU, nX)
    cd, Xd, Ud = nw.drop_last_feature(c, Xn, Un)
    F = nU + nX
    assert (0 if cd["U"] is None else cd["U"].shape[1]) + (0 if cd["X"] is None else cd["X"].shape[1]) == F - 1
    assert (cd["X"] is None) == (Xd is None) and (cd["U"] is None) == (Ud is None)
    lv = nw.levels(form)[0]
    for s in range(c["S"]):
        ys = float(c["yScale"][s])
        lit = nr.literal(c, s, Xn, Un, nw.M, form, lv)
        st = nr.structured(c, s, Xn, Un, nw.M, form, lv)
        drop = nr.literal(cd, s, Xd, Ud, nw.M, form, lv)
        moves = np.zeros((len(lv), 3))
        for l in range(len(lv)):
            what = f"nU={nU} nX={nX} {form} s={s} l={l}"
            _close(st[0][:, l], lit[0][:, l], ys, what + " mean", mean=True)
            _close(st[1][:, l], lit[1][:, l], ys, what + " var")
            _close(st[2][l], lit[2][l], ys, what + " cov")
            bm, bv, bc = nw.tight_bounds(lit[0][:, l], lit[1][:, l], lit[2][l], ys)
            moves[l] = (np.max(np.abs(drop[0][:, l] - lit[0][:, l])) / bm, np.max(np.abs(drop[1][:, l] - lit[1][:, l]) / bv),
                        np.max(np.abs(drop[2][l] - lit[2][l])) / bc)
        print(f"nU={nU} nX={nX} {form} s={s}: move / tight bound (mean, var, cov) per level", moves.tolist())
        assert np.all(moves >= 1e6), moves                               # every level, not only the sample's largest


@pytest.mark.parametrize("place", nw.PAD_PLACES)
def test_constant_columns_leave_the_restatement_where_it_was(place):
    """the reference side of the GPU test's padding identity, at the widest padding (F = 32): a constant column adds
    ((c - c) / l)^2 = 0 to every pair"""
    c = nw.width_case(2, 3)
    Xn, Un = nw.width_new(2, 3)
    k = nw.PAD_COUNTS[-1]
    cp, Xp, Up = nw.pad_constant(c, Xn, Un, k, place)
    nUp, nXp = cp["U"].shape[1], cp["X"].shape[1]
    assert nUp + nXp == 32 and Xp.shape == (nw.M, nXp) and Up.shape == (nw.M, nUp, c["S"])
    assert cp["uyLS"].shape == (nUp, c["S"]) and cp["xyLS"].shape == (nXp, c["S"])
    new = (cp["U"][:, 2:, :], Up[:, 2:, :]) if place == "U" else \
        ((cp["X"][:, 3:], Xp[:, 3:]) if place == "X back" else (cp["X"][:, :k], Xp[:, :k]))
    for a in new:                                                        # constant down every column, distinct and nonzero
        col = a.reshape(a.shape[0], k, -1)
        assert np.all(col == col[:1]) and np.all(col != 0.0) and len(np.unique(col[0, :, 0])) == k
    assert np.array_equal(new[0][0], new[1][0])
    kept = cp["X"][:, k:] if place == "X front" else cp["X"][:, :3]
    assert np.array_equal(kept, c["X"]) and np.array_equal(cp["U"][:, :2, :], c["U"])
    lv = nw.levels("contrast")[0]
    for s in range(c["S"]):
        plain = nr.literal(c, s, Xn, Un, nw.M, "contrast", lv)
        padded = nr.literal(cp, s, Xp, Up, nw.M, "contrast", lv)
        ys = float(c["yScale"][s])
        for l in range(len(lv)):                  # NumPy sums the 32 squares in another order than the 5: the tight bound, not bits
            _close(padded[0][:, l], plain[0][:, l], ys, f"{place} s={s} l={l} mean", mean=True)
            _close(padded[1][:, l], plain[1][:, l], ys, f"{place} s={s} l={l} var")
            _close(padded[2][l], plain[2][l], ys, f"{place} s={s} l={l} cov")
