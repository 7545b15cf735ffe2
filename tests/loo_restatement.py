"""Host restatement of the leave-one-out (LOO) predictive checks of the outcome model Y ~ N(0, A), A = orc.y_cov(...)
(test infrastructure; Rasmussen & Williams §5.4.2).  Two independent computations:

  closed_form   looMean_i = Y_i - alpha_i / c_i, looVar_i = 1 / c_i with alpha = inv(A) Y, c = diag(inv(A));
  refit         literally: delete row and column i, condition Y_i on the other n - 1 observations.

Both return (mean, var, lpd) of shape (n,) for one posterior sample."""
import math

import numpy as np

import gpslc_oracle as orc

LOG2PI = math.log(2.0 * math.pi)


def cov_of(case, p, X=None):
    """A of posterior sample `p` (cases.samples_of) on the case's data; `X` overrides the case's covariates"""
    X = case["X"] if X is None else X
    return orc.y_cov(p.uyLS, p.xyLS, p.tyLS, p.yScale, p.yNoise, p.U, X, case["T"])


def _lpd(Y, mean, var):
    return -0.5 * LOG2PI - 0.5 * np.log(var) - 0.5 * (Y - mean) ** 2 / var


def closed_form(A, Y):
    Ai = np.linalg.inv(A)
    c = np.diag(Ai).copy()
    alpha = Ai @ Y
    mean, var = Y - alpha / c, 1.0 / c
    return mean, var, _lpd(Y, mean, var)


def refit(A, Y):
    n = A.shape[0]
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        if n == 1:
            mean[i], var[i] = 0.0, A[0, 0]
            continue
        k = A[keep, i]
        sol = np.linalg.solve(A[np.ix_(keep, keep)], np.column_stack([Y[keep], k]))
        mean[i] = k @ sol[:, 0]
        var[i] = A[i, i] - k @ sol[:, 1]
    return mean, var, _lpd(Y, mean, var)


def tolerance(A):
    """The bound of the GPU tests for one sample: max(1e-10, 1e-14 cond(A)) — 1e-10 is test_gpu_estimation's bound for y_logpdf
    against the oracle, the cond term follows cases.draw_bounds.  Returns (tol, cond)."""
    cond = float(np.linalg.cond(A))
    return max(1e-10, 1e-14 * cond), cond


def errors(got, ref, Y):
    """(looVar relative, looMean absolute / max|Y|, looLpd absolute / (1 + max_i zscore_i^2)) of got = (mean, var, lpd) against
    ref: each is compared with the sample's `tol`."""
    gm, gv, gl = got
    rm, rv, rl = ref
    z2 = float(np.max((Y - rm) ** 2 / rv))
    ymax = max(float(np.max(np.abs(Y))), np.finfo(float).tiny)
    return (float(np.max(np.abs(gv - rv) / rv)), float(np.max(np.abs(gm - rm))) / ymax,
            float(np.max(np.abs(gl - rl))) / (1.0 + z2))


def expected(case, samples=None, X=None, Y=None):
    """Per posterior sample of `samples` (default: all): dict(A, tol, cond, closed, refit) on the case's data or the overrides"""
    import cases
    Y = np.asarray(case["Y"] if Y is None else Y, dtype=np.float64)
    smp = cases.samples_of(case)
    out = {}
    for s in (range(case["S"]) if samples is None else samples):
        A = cov_of(case, smp[s], X)
        tol, cond = tolerance(A)
        out[s] = dict(A=A, tol=tol, cond=cond, closed=closed_form(A, Y), refit=refit(A, Y))
    return out
