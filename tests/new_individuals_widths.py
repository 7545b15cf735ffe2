"""Cases for predictions for new individuals over the feature width F = nU + nX (test infrastructure beside
new_individuals_restatement.py; shared by tests/test_new_individuals_widths.py on the CPU and tests/test_gpu_new_individuals_widths.py
on the GPU).

new_mean_mfma_kernel<FREG, FORM> is compiled over pair_mfma_freg_ladder: FREG = 4, 6, 8, 10, 12 registers for the features of a
lane's rows, 0 = features from LDS for F >= 13, times three level forms.  WIDTHS has both edges of every rung, the first F served
from LDS, MAXF = 32, and U-only, X-only, U-heavy and X-heavy mixes.

With standard-normal features and make_case's lengthscales the kernel value B*_ij / yScale = exp(-sum_f ((w*_if - w_jf) / l_f)^2)
vanishes as F grows (median 1e-7 at F = 8, 1e-14 at F = 13): A becomes the identity and any kernel passes.  `normalise` rescales
every sample's lengthscales by one factor so that sum_f 1 / l_f^2 = 0.5: the expected exponent E sum_f (w*_f - w_f)^2 / l_f^2 =
2 sum_f 1 / l_f^2 is then 1 at every width."""
import functools

import numpy as np

import cases
import new_individuals_restatement as nr

N, M, S, L = 129, 130, 2, 3          # two training tiles, the second with one live row; two row tiles of new individuals

# (nU, nX): F and the FREG rung that serves it
WIDTHS = [(1, 0), (0, 1),                                   # F = 1   rung 4
          (2, 2),                                           # F = 4   rung 4
          (2, 4),                                           # F = 6   rung 6
          (3, 4), (2, 6),                                   # F = 7, 8   rung 8
          (4, 5), (2, 8),                                   # F = 9, 10  rung 10
          (5, 6), (4, 8),                                   # F = 11, 12 rung 12
          (5, 8), (0, 13), (13, 0),                         # F = 13  rung 0 (features from LDS)
          (8, 24), (24, 8), (0, 32), (32, 0)]               # F = 32 = MAXF  rung 0
ONE_PER_RUNG = [(2, 2), (2, 4), (2, 6), (2, 8), (4, 8), (5, 8), (8, 24)]
PAD_COUNTS = (1, 2, 4, 6, 8, 27)     # constant columns added to the F = 5 case: F = 6, 7, 9, 11, 13, 32, one on every rung
PAD_PLACES = ("X back", "X front", "U")


def freg_rung(F):
    """pair_mfma_freg_ladder's choice"""
    return next((r for r in (4, 6, 8, 10, 12) if F <= r), 0)


def shape_of(nU, nX):
    return {(True, True): "UX", (True, False): "U", (False, True): "X", (False, False): "T"}[(nU > 0, nX > 0)]


def normalise(case):
    """A new case whose lengthscales are rescaled, one factor per posterior sample, to sum_f 1 / l_f^2 = 0.5"""
    c = dict(case)
    tot = np.zeros(case["S"])
    for k in ("uyLS", "xyLS"):
        if case[k] is not None:
            tot += np.sum(1.0 / case[k] ** 2, axis=0)
    f = np.sqrt(2.0 * tot)
    for k in ("uyLS", "xyLS"):
        if case[k] is not None:
            c[k] = np.asfortranarray(case[k] * f[None, :])
    return c


@functools.lru_cache(maxsize=None)
def width_case(nU, nX, n=N, S=S):
    return normalise(cases.make_case(n, shape_of(nU, nX), False, S=S, nU=nU, nX=nX, seed=300 + nU + nX))


@functools.lru_cache(maxsize=None)
def width_new(nU, nX, m=M):
    """(Xnew, Unew) of the width's case"""
    return nr.new_individuals(width_case(nU, nX), m, seed=1)


def levels(form, count=L):
    """[(a, b or None)], doT, base or None"""
    lv = nr.pairs(form, count)
    return lv, np.array([a for a, _ in lv]), (np.array([b for _, b in lv]) if form == "contrast" else None)


def drop_last_feature(case, Xn, Un):
    """(case, Xnew, Unew) without the last feature column — the last X column, or the last U column of a model without X — in
    the training data, the new individuals and the lengthscales; a side left without columns becomes None"""
    c = dict(case)
    side = ("X", "xyLS") if case["X"] is not None else ("U", "uyLS")
    cut = lambda a: None if a.shape[1] == 1 else np.asfortranarray(a[:, :-1])       # noqa: E731
    c[side[0]] = cut(case[side[0]])
    c[side[1]] = None if c[side[0]] is None else np.asfortranarray(case[side[1]][:-1])
    if side[0] == "X":
        Xn = cut(Xn)
    else:
        Un = cut(Un)
    c["shape"] = shape_of(0 if c["U"] is None else c["U"].shape[1], 0 if c["X"] is None else c["X"].shape[1])
    return c, Xn, Un


def pad_constant(case, Xn, Un, k, place):
    """(case, Xnew, Unew) with k constant feature columns added: column j holds the value PAD_VALUE(j) != 0 for every training
    and every new individual (and in every sample's block of U), with a lengthscale of its own.  `place`: behind the X columns,
    in front of them, or behind the U columns.  Nothing else changes: the other lengthscales are not rescaled."""
    c = dict(case)
    n, m, S_ = case["n"], Xn.shape[0], case["S"]
    val = np.array([(-1.0) ** j * (0.75 + 0.5 * j) for j in range(k)])
    ls = np.array([[0.3 + 0.7 * j + 0.11 * s for s in range(S_)] for j in range(k)])
    if place == "U":
        c["U"] = np.asfortranarray(np.concatenate([case["U"], np.broadcast_to(val[None, :, None], (n, k, S_))], axis=1))
        Un = np.asfortranarray(np.concatenate([Un, np.broadcast_to(val[None, :, None], (m, k, S_))], axis=1))
        c["uyLS"] = np.asfortranarray(np.concatenate([case["uyLS"], ls], axis=0))
        return c, Xn, Un
    parts = (lambda a, b: [a, b]) if place == "X back" else (lambda a, b: [b, a])
    c["X"] = np.concatenate(parts(case["X"], np.broadcast_to(val[None, :], (n, k))), axis=1)
    Xn = np.asfortranarray(np.concatenate(parts(Xn, np.broadcast_to(val[None, :], (m, k))), axis=1))
    c["xyLS"] = np.asfortranarray(np.concatenate(parts(case["xyLS"], ls), axis=0))
    return c, Xn, Un


def median_kernel(case, s, Xn, Un):
    """median over the (new, training) pairs of B*_ij / yScale"""
    m = (Xn if Xn is not None else Un).shape[0]
    return float(np.median(nr.blocks(case, s, Xn, Un, m)[1]) / case["yScale"][s])


def tight_bounds(ref_mean, ref_var, ref_cov, ys):
    """The tight bounds of test_gpu_contrast._check as tests/test_gpu_new_individuals.py applies them to one (sample, level):
    mean 1e-9 max|ref| + 1e-13 (a scalar), var 1e-9 |ref| + 1e-12 yScale per element, cov 1e-9 max|block| + 1e-12 yScale"""
    return (1e-9 * float(np.max(np.abs(ref_mean))) + 1e-13, 1e-9 * np.abs(ref_var) + 1e-12 * ys,
            1e-9 * float(np.max(np.abs(ref_cov))) + 1e-12 * ys)
