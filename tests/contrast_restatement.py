"""Dense NumPy restatement of the estimation path for a contrast between two scalar intervention levels a and b.

The reference's estimand is f(doT) - f(T) (src/estimation.jl:46-47).  A contrast is f(a) - f(b): the joint Gaussian-process
prior over (f(T), f(a 1), f(b 1)) is built from the oracle's own pieces exactly as src/likelihood.jl:24-39 builds its blocks,
conditioned on Y, and the difference of the two counterfactual blocks is taken:

    D        = CovWWs_a' - CovWWs_b'
    MeanITE  = D (CovWWp \\ Y)
    CovITE   = (Kaa - Kab - Kba + Kbb) - D (CovWWp \\ D'),   Symmetric(.) + pred_noise I   (src/estimation.jl:82)

This is the literal side (dense n x n blocks, LAPACK solves); the library is the structured side.
"""
import numpy as np

import gpslc_oracle as orc


def contrast_blocks(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a, b):
    """(CovWWp, CovWWs_a, CovWWs_b, Kaa, Kab, Kba, Kbb): the blocks of the joint prior, src/likelihood.jl:24-39 with a second
    counterfactual column."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    Tm = orc._as_2d(T)
    base = np.zeros((n, n))
    if U is not None:
        Um = orc._as_2d(U)
        base = base + orc.rbf_kernel_log(Um, Um, np.atleast_1d(uyLS))
    if X is not None:
        Xm = orc._as_2d(X)
        base = base + orc.rbf_kernel_log(Xm, Xm, np.atleast_1d(xyLS))
    av = np.full((n, 1), float(a))
    bv = np.full((n, 1), float(b))
    CovWW = orc.process_cov(base + orc.rbf_kernel_log(Tm, Tm, tyLS), yScale, 0.0)
    CovWWp = CovWW + yNoise * np.eye(n)
    CovWWs_a = orc.process_cov(base + orc.rbf_kernel_log(Tm, av, tyLS), yScale, 0.0)
    CovWWs_b = orc.process_cov(base + orc.rbf_kernel_log(Tm, bv, tyLS), yScale, 0.0)
    Kaa = orc.process_cov(base + orc.rbf_kernel_log(av, av, tyLS), yScale, 0.0)
    Kab = orc.process_cov(base + orc.rbf_kernel_log(av, bv, tyLS), yScale, 0.0)
    Kba = orc.process_cov(base + orc.rbf_kernel_log(bv, av, tyLS), yScale, 0.0)
    Kbb = orc.process_cov(base + orc.rbf_kernel_log(bv, bv, tyLS), yScale, 0.0)
    return CovWWp, CovWWs_a, CovWWs_b, Kaa, Kab, Kba, Kbb


def conditional_ite_contrast(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a, b):
    """MeanITE (n,), CovITE (n, n) of f(a) - f(b) given Y; no jitter, like src/estimation.jl:36-50."""
    CovWWp, Ksa, Ksb, Kaa, Kab, Kba, Kbb = contrast_blocks(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a, b)
    D = Ksa.T - Ksb.T
    MeanITE = D @ orc._sym_solve(CovWWp, np.asarray(Y, dtype=np.float64))
    CovITE = (((Kaa - Kab) - Kba) + Kbb) - D @ orc._sym_solve(CovWWp, D.T)
    return MeanITE, CovITE


def ite_distributions_contrast(samples, X, T, Y, a, b, pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """src/estimation.jl:66-86 for the contrast a against b."""
    n = np.asarray(Y).shape[0]
    S = len(samples)
    MeanITEs = np.zeros((S, n))
    CovITEs = np.zeros((S, n, n))
    for idx, p in enumerate(samples):
        m, C = conditional_ite_contrast(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, a, b)
        MeanITEs[idx] = m
        CovITEs[idx] = orc._symmetric_upper(C) + np.eye(n) * pred_noise
    return MeanITEs, CovITEs


def expected_contrast(case, A, B, samples=None, pred_noise=orc.PREDICTION_COVARIANCE_NOISE, want_cov=True):
    """Restatement outputs for every (sample, level) of the pairs (A[l], B[l]); `samples` restricts to those sample indices
    (the arrays keep the call's sample axis, other samples stay zero).  want_cov=False drops the (S, L, n, n) array."""
    from cases import samples_of
    smp = samples_of(case)
    S, n = case["S"], case["n"]
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    B = np.broadcast_to(np.asarray(B, dtype=np.float64), A.shape)
    L = A.shape[0]
    idx = list(range(S)) if samples is None else list(samples)
    meanITE = np.zeros((n, S, L))
    covITE = np.zeros((S, L, n, n)) if want_cov else None
    mS = np.zeros((S, L))
    vS = np.zeros((S, L))
    for l in range(L):
        M, Cv = ite_distributions_contrast([smp[s] for s in idx], case["X"], case["T"], case["Y"], A[l], B[l], pred_noise)
        for k, s in enumerate(idx):
            meanITE[:, s, l] = M[k]
            if want_cov:
                covITE[s, l] = Cv[k]
            mS[s, l], vS[s, l] = orc.conditional_sate(M[k], Cv[k])
    return dict(meanITE=meanITE, covITE=covITE, meanSATE=mS, varSATE=vS)


def pairs(case, L):
    """L test pairs (A, B): (1, 0) / (0, 1) alternating for a binary treatment; for a continuous one pairs at least 0.25 apart
    (the smallest tyLS cases.make_case produces: closer pairs cancel in r^a - r^b and 1 - rho) — (0.6, -0.4), the 0.8 / 0.2
    quantiles of T, then a sweep of levels over the range of T against baselines that keep that distance."""
    if case["binary_t"]:
        A = np.array([float((l + 1) % 2) for l in range(L)])
        return A, 1.0 - A
    T = case["T"]
    q8, q2 = float(np.quantile(T, 0.8)), float(np.quantile(T, 0.2))
    if q8 - q2 < 0.25:
        q8 = q2 + 0.25
    A = np.empty(L)
    B = np.empty(L)
    for l in range(L):
        if l == 0:
            A[l], B[l] = 0.6, -0.4
        elif l == 1:
            A[l], B[l] = q8, q2
        else:
            A[l] = -1.5 + 3.0 * (l - 2) / max(L - 3, 1)
            B[l] = A[l] - (0.25 + 0.5 * ((l * 7) % 5) / 4.0) if l % 2 else A[l] + (0.25 + 0.5 * ((l * 3) % 5) / 4.0)
    return A, B
