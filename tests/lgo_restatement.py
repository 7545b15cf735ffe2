"""Host restatement of the leave-group-out (LGO) predictive checks of the outcome model Y ~ N(0, A), A = orc.y_cov(...)
(test infrastructure; Rasmussen & Williams §5.4.2 in block form).  Two independent computations per posterior sample:

  closed_form   alpha = inv(A) Y and, per group I, C = inv(A)[I, I] through its Cholesky factor:
                mean_I = Y_I - inv(C) alpha_I, var = diag(inv(C)), lpd = -(m/2) log 2 pi + log det(C)/2 - alpha_I' inv(C) alpha_I / 2;
  refit         literally: delete the group's rows and columns, condition Y_I on the rest, and take the joint Gaussian density
                of Y_I (nobody left: the prior N(0, A)).

Both return (mean (n,), var (n,), lpd (G,)); refit also returns q (G,), the Mahalanobis distance of every group.  Groups are
given as labels in [0, G); a group's members are taken in ascending row order."""
import math

import numpy as np

from loo_restatement import cov_of

LOG2PI = math.log(2.0 * math.pi)


def members_of(labels):
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == g) for g in range(int(labels.max()) + 1)]


def closed_form(A, Y, labels):
    n = A.shape[0]
    groups = members_of(labels)
    Ai = np.linalg.inv(A)
    alpha = Ai @ Y
    mean, var, lpd = np.empty(n), np.empty(n), np.empty(len(groups))
    conds = np.empty(len(groups))
    for g, I in enumerate(groups):
        C = Ai[np.ix_(I, I)]
        conds[g] = np.linalg.cond(C)
        R = np.linalg.cholesky(C)
        z = np.linalg.solve(R, alpha[I])
        mean[I] = Y[I] - np.linalg.solve(R.T, z)
        Ri = np.linalg.inv(R)
        var[I] = np.sum(Ri * Ri, axis=0)
        lpd[g] = -0.5 * len(I) * LOG2PI + np.sum(np.log(np.diag(R))) - 0.5 * (z @ z)
    return (mean, var, lpd), conds


def refit(A, Y, labels):
    n = A.shape[0]
    groups = members_of(labels)
    mean, var, lpd, q = np.empty(n), np.empty(n), np.empty(len(groups)), np.empty(len(groups))
    for g, I in enumerate(groups):
        keep = np.ones(n, dtype=bool)
        keep[I] = False
        if not keep.any():
            mu, cov = np.zeros(len(I)), A[np.ix_(I, I)]
        else:
            K = A[np.ix_(keep, I)]
            sol = np.linalg.solve(A[np.ix_(keep, keep)], np.column_stack([Y[keep], K]))
            mu = K.T @ sol[:, 0]
            cov = A[np.ix_(I, I)] - K.T @ sol[:, 1:]
            cov = 0.5 * (cov + cov.T)
        L = np.linalg.cholesky(cov)
        r = np.linalg.solve(L, Y[I] - mu)
        q[g] = r @ r
        mean[I], var[I] = mu, np.diag(cov)
        lpd[g] = -0.5 * len(I) * LOG2PI - np.sum(np.log(np.diag(L))) - 0.5 * q[g]
    return (mean, var, lpd), q


def tolerance(A, cond_c):
    """The bound of one sample: max(1e-10, 1e-14 cond(A) max_g cond(C_g)) — the bound of loo_restatement.tolerance for the
    entries of W, times the condition of the block that is then solved with.  Returns (tol, cond(A))."""
    cond = float(np.linalg.cond(A))
    return max(1e-10, 1e-14 * cond * float(np.max(cond_c))), cond


def errors(got, ref, q, Y, labels):
    """(lgoVar relative, lgoMean absolute / max|Y|, lgoLpd absolute / (m_g + q_g)) of got = (mean, var, lpd) against ref; q: the
    refit's Mahalanobis distances.  Each is compared with the sample's `tol`."""
    gm, gv, gl = got
    rm, rv, rl = ref
    m = np.bincount(np.asarray(labels), minlength=len(rl)).astype(np.float64)
    ymax = max(float(np.max(np.abs(Y))), np.finfo(float).tiny)
    with np.errstate(invalid="ignore"):
        ev = float(np.max(np.abs(gv - rv) / rv))
        em = float(np.max(np.abs(gm - rm))) / ymax
        el = float(np.max(np.abs(gl - rl) / (m + q)))
    return tuple(e if np.isfinite(e) else np.inf for e in (ev, em, el))


def expected(case, labels, samples=None, X=None, Y=None):
    """Per posterior sample of `samples` (default: all): dict(A, tol, cond, cond_c, closed, refit, q) on the case's data or the
    overrides, for the grouping `labels`"""
    import cases
    Y = np.asarray(case["Y"] if Y is None else Y, dtype=np.float64)
    smp = cases.samples_of(case)
    out = {}
    for s in (range(case["S"]) if samples is None else samples):
        A = cov_of(case, smp[s], X)
        closed, cond_c = closed_form(A, Y, labels)
        ref, q = refit(A, Y, labels)
        tol, cond = tolerance(A, cond_c)
        out[s] = dict(A=A, tol=tol, cond=cond, cond_c=float(np.max(cond_c)), closed=closed, refit=ref, q=q)
    return out


# ---- the labellings of the tests --------------------------------------------------------------------------------------
def singletons(n):
    return np.arange(n, dtype=np.int32)


def one_group(n):
    return np.zeros(n, dtype=np.int32)


def mod7(n):
    """scattered members across tile rows, sizes not multiples of 16 or 4 (fewer than 7 individuals: compacted)"""
    return np.unique(np.arange(n) % 7, return_inverse=True)[1].astype(np.int32)


def blocks_of(n, size):
    return (np.arange(n) // size).astype(np.int32)


def with_block(n, lo, hi, rest=17):
    """rows lo .. hi - 1 as one group (the last label), the others in contiguous blocks of `rest`"""
    lab = np.empty(n, dtype=np.int64)
    others = np.r_[np.arange(0, lo), np.arange(hi, n)]
    lab[others] = np.arange(len(others)) // rest
    lab[lo:hi] = (lab[others].max() + 1) if len(others) else 0
    return lab.astype(np.int32)
