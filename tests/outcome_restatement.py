"""Dense NumPy restatement of the estimation path for the potential outcome mu_i(a) = f_i(a): the response surface itself at a
scalar level a (everybody set to a) or at a per-individual level d (individual i set to d_i).

Nothing is derived here: the outcome is the reference's own counterfactual block.  likelihoodDistribution
(src/likelihood.jl:27-49, oracle/gpslc_oracle.likelihood_distribution; tests/vector_restatement.likelihood_distribution_vec for a
vector) forms CovWWs = Cov(Y, f(doT)), CovWsWs = Cov(f(doT), f(doT)) and

    CovC22 = CovWsWs - CovWWs' CovWWp^-1 CovWWs,

the posterior covariance of f(doT); conditionalITE only uses it inside C11 - C12 - C21 + C22.  So

    MeanOutcome = CovWWs' (CovWWp \\ Y)
    CovOutcome  = CovC22,   Symmetric(.) + pred_noise I   (src/estimation.jl:82, as ite_distributions_slope adds it)

This is the literal side (dense n x n blocks, LAPACK solves); the library is the structured side.  Also here: the
dense cross-level covariance of the weighted outcomes of a sweep, and the library's structured formulas in NumPy.
"""
import numpy as np
from scipy.linalg import solve_triangular

import gpslc_oracle as orc
import vector_restatement as vr

PN = orc.PREDICTION_COVARIANCE_NOISE


def _base_log(U, uyLS, X, xyLS, n):
    base = np.zeros((n, n))
    if U is not None:
        Um = orc._as_2d(U)
        base = base + orc.rbf_kernel_log(Um, Um, np.atleast_1d(uyLS))
    if X is not None:
        Xm = orc._as_2d(X)
        base = base + orc.rbf_kernel_log(Xm, Xm, np.atleast_1d(xyLS))
    return base


def conditional_outcome(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a):
    """Mean (n,), Cov (n, n) of f(a) given Y at the scalar level a; no jitter, like src/estimation.jl:36-50."""
    Y, _, CovWWs, CovWWp, _, _, _, C22 = orc.likelihood_distribution(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a)
    return CovWWs.T @ orc._sym_solve(CovWWp, Y), C22


def conditional_outcome_vec(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, d):
    """The same at the per-individual level d (n,)."""
    Y, _, CovWWs, CovWWp, _, _, _, C22 = vr.likelihood_distribution_vec(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, d)
    return CovWWs.T @ orc._sym_solve(CovWWp, Y), C22


def ite_distributions_outcome(samples, X, T, Y, a, pred_noise=PN):
    """src/estimation.jl:66-86 for the outcome at a: a scalar, or a vector of n per-individual values."""
    n = np.asarray(Y).shape[0]
    S = len(samples)
    fn = conditional_outcome if np.ndim(a) == 0 else conditional_outcome_vec
    Means = np.zeros((S, n))
    Covs = np.zeros((S, n, n))
    for idx, p in enumerate(samples):
        m, C = fn(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, a)
        Means[idx] = m
        Covs[idx] = orc._symmetric_upper(C) + np.eye(n) * pred_noise
    return Means, Covs


def _expected(case, levels, samples, pred_noise, want_cov):
    from cases import samples_of
    smp = samples_of(case)
    S, n, L = case["S"], case["n"], len(levels)
    idx = list(range(S)) if samples is None else list(samples)
    meanITE = np.zeros((n, S, L))
    covITE = np.zeros((S, L, n, n)) if want_cov else None
    mS = np.zeros((S, L))
    vS = np.zeros((S, L))
    for l in range(L):
        M, Cv = ite_distributions_outcome([smp[s] for s in idx], case["X"], case["T"], case["Y"], levels[l], pred_noise)
        for k, s in enumerate(idx):
            meanITE[:, s, l] = M[k]
            if want_cov:
                covITE[s, l] = Cv[k]
            mS[s, l], vS[s, l] = orc.conditional_sate(M[k], Cv[k])
    return dict(meanITE=meanITE, covITE=covITE, meanSATE=mS, varSATE=vS)


def expected_outcome(case, A, samples=None, pred_noise=PN, want_cov=True):
    """Restatement outputs for every (sample, level) of the scalar levels A; `samples` restricts to those sample indices (the
    arrays keep the call's sample axis, other samples stay zero).  want_cov=False drops the (S, L, n, n) array."""
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    return _expected(case, [float(a) for a in A], samples, pred_noise, want_cov)


def expected_outcome_vec(case, D, samples=None, pred_noise=PN, want_cov=True):
    """The same for the (L, n) per-individual levels D."""
    D = np.atleast_2d(np.asarray(D, dtype=np.float64))
    return _expected(case, [D[l] for l in range(D.shape[0])], samples, pred_noise, want_cov)


def levels(case, L):
    """L scalar levels: for a continuous treatment the case's own two, then a sweep over [-1.5, 1.5]; for a binary one the two
    treatment values, the midpoint and values between."""
    if case["binary_t"]:
        return np.array([(0.0, 1.0, 0.5, 0.3, 0.8)[l % 5] + 0.01 * (l // 5) for l in range(L)])
    return np.concatenate([case["doTs"], np.linspace(-1.5, 1.5, max(L - 2, 0))])[:L].copy()


def literal_outcome_curve(case, s, doTs, W, pred_noise=PN):
    """Dense mean (L, G) and joint covariance (L, L, G) of tau_l = w_g' f(a_l) for posterior sample s: every (l, l') block
    Cov(f(a_l), f(a_l') | Y) = B rho(a_l, a_l') - D_l A^-1 D_l'' is formed n x n and summed against the weights."""
    from cases import samples_of
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    p = samples_of(case)[s]
    X, T, Y = case["X"], case["T"], np.asarray(case["Y"], dtype=np.float64)
    n = Y.shape[0]
    L, G = doTs.shape[0], W.shape[0]
    base = _base_log(p.U, p.uyLS, X, p.xyLS, n)
    mean, cov = np.zeros((L, G)), np.zeros((L, L, G))
    ww = np.sum(W * W, axis=1)
    blocks = [orc.likelihood_distribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, a) for a in doTs]
    CovWWp = blocks[0][3]
    for l in range(L):
        Dl = blocks[l][2].T
        for lp in range(l + 1):
            Dlp = blocks[lp][2].T
            av, bv = np.full((n, 1), float(doTs[l])), np.full((n, 1), float(doTs[lp]))
            Kab = orc.process_cov(base + orc.rbf_kernel_log(av, bv, p.tyLS), p.yScale, 0.0)
            Cb = Kab - Dl @ orc._sym_solve(CovWWp, Dlp.T)
            if l == lp:
                Cb = orc._symmetric_upper(Cb)
                mean[l] = W @ (Dl @ orc._sym_solve(CovWWp, Y))
            v = np.einsum("gi,ij,gj->g", W, Cb, W)
            cov[l, lp] = cov[lp, l] = v + (pred_noise * ww if l == lp else 0.0)
    return mean, cov


def expected_outcome_curve(case, doTs, W, pred_noise=PN, samples=None):
    """literal_outcome_curve for every sample: mean (S, L, G), cov (S, L, L, G); `samples` restricts (the others stay zero)."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(W)
    S, L, G = case["S"], doTs.shape[0], W.shape[0]
    mean, cov = np.zeros((S, L, G)), np.zeros((S, L, L, G))
    for s in (range(S) if samples is None else samples):
        mean[s], cov[s] = literal_outcome_curve(case, s, doTs, W, pred_noise)
    return dict(mean=mean, cov=cov)


def _factor(case, s):
    from cases import samples_of
    p = samples_of(case)[s]
    n, T, Y = case["n"], np.asarray(case["T"], dtype=np.float64), np.asarray(case["Y"], dtype=np.float64)
    om = 1.0 / (p.tyLS * p.tyLS)
    B = p.yScale * np.exp(_base_log(p.U, p.uyLS, case["X"], p.xyLS, n))
    K = B * np.exp(-((T[:, None] - T[None, :]) ** 2) * om)
    Lc = np.linalg.cholesky(K + p.yNoise * np.eye(n))
    return p, T, om, B, Lc, solve_triangular(Lc, Y, lower=True)


def structured_outcome_curve(case, s, doTs, w, pred_noise=PN):
    """The library's formulas for one sample and weight vector in NumPy: mean (L,), cov (L, L) of w' f(a_l) — no n x n block
    of the outcome is formed: c_l = r^l .* (B w), v_l = L^-1 c_l, P_ll' = rho(a_l, a_l') beta, beta = w . (B w)."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    p, T, om, B, Lc, z = _factor(case, s)
    bw = B @ w
    beta = float(w @ bw)
    L = doTs.shape[0]
    V = [solve_triangular(Lc, np.exp(-((T - a) ** 2) * om) * bw, lower=True) for a in doTs]
    mean = np.array([float(v @ z) for v in V])
    cov = np.zeros((L, L))
    for l in range(L):
        for lp in range(l + 1):
            d = doTs[l] - doTs[lp]
            P = np.exp(-(d * d) * om) * beta
            cov[l, lp] = cov[lp, l] = (P - float(V[l] @ V[lp])) + (pred_noise * float(w @ w) if l == lp else 0.0)
    return mean, cov


def structured_outcome_average(case, s, a, pred_noise=PN):
    """The plain form's formulas: (mean, var) of the 1/n average, mean = w . z / n and
    var = (sum(B) - w . w + n pred_noise) / n^2 with w = L^-1 (r^a .* bsum)."""
    n = case["n"]
    m, c = structured_outcome_curve(case, s, [a], np.full(n, 1.0), pred_noise=0.0)
    return m[0] / n, (c[0, 0] + n * pred_noise) / (n * n)


def structured_outcome_vec(case, s, d, pred_noise=PN):
    """The vector level's formulas: (MeanOutcome (n,), mean, var) with g_ji = rho(T_j, d_i), h_ij = rho(d_i, d_j):
    MeanOutcome_i = sum_j B_ij g_ji alpha_j, c_j = sum_i B_ij g_ji, w = L^-1 c, mean = w . z / n and
    var = (sum_ij B_ij h_ij - w . w + n pred_noise) / n^2."""
    d = np.asarray(d, dtype=np.float64)
    n = case["n"]
    p, T, om, B, Lc, z = _factor(case, s)
    Gm = np.exp(-((T[None, :] - d[:, None]) ** 2) * om)          # [i, j] = g_ji = rho(T_j, d_i)
    H = np.exp(-((d[:, None] - d[None, :]) ** 2) * om)
    D = B * Gm
    alpha = solve_triangular(Lc.T, z, lower=False)
    w = solve_triangular(Lc, D.sum(axis=0), lower=True)
    return D @ alpha, float(w @ z) / n, (float(np.sum(B * H)) - float(w @ w) + n * pred_noise) / (n * n)


# (n, shape, seed, levels, pred_noise values): the draw cases of tests/test_gpu_outcome.py.  tests/test_outcome.py checks on the
# CPU that every jitter-free restatement covariance of these cases has its smallest eigenvalue >= -1e-12 yScale (DESIGN.md §16
# lists the measured values).
DRAW_CASES = [(129, "UX", 61, 1), (200, "UX", 61, 3), (150, "T", 61, 2)]
