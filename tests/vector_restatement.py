"""Dense NumPy restatement of the estimation path for a per-individual intervention vector d.

The reference declares `Intervention = Union{Bool, Vector{Bool}, Float64, Vector{Float64}}` (src/types.jl:138-143) but its
likelihoodDistribution builds `fill(doT, n)` (src/likelihood.jl:27-28), which has no rbfKernelLog method for a vector.  This
module is oracle/gpslc_oracle.likelihood_distribution with that one line changed — the column d in place of fill(doT, n) —
and the estimation functions of the oracle on top of it.  For d = fill(x, n) it is the oracle itself, bit for bit.
"""
import numpy as np

import gpslc_oracle as orc


def likelihood_distribution_vec(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, d):
    """src/likelihood.jl:8-174 with d (n,) replacing fill(doT, n)."""
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
    doTv = np.asarray(d, dtype=np.float64).reshape(n, 1)               # the one changed line (:27-28)
    tyCovLog = orc.rbf_kernel_log(Tm, Tm, tyLS)
    tyCovLogS = orc.rbf_kernel_log(Tm, doTv, tyLS)
    tyCovLogSS = orc.rbf_kernel_log(doTv, doTv, tyLS)

    CovWW = orc.process_cov(base + tyCovLog, yScale, 0.0)
    CovWWp = CovWW + yNoise * np.eye(n)
    CovWWs = orc.process_cov(base + tyCovLogS, yScale, 0.0)
    CovWsWs = orc.process_cov(base + tyCovLogSS, yScale, 0.0)

    CovWWpInvCovWW = orc._sym_solve(CovWWp, CovWW)
    CovWWpInvCovWWs = orc._sym_solve(CovWWp, CovWWs)

    CovC11 = CovWW - CovWW @ CovWWpInvCovWW
    CovC12 = CovWWs - CovWW @ CovWWpInvCovWWs
    CovC21 = CovWWs.T - CovWWs.T @ CovWWpInvCovWW
    CovC22 = CovWsWs - CovWWs.T @ CovWWpInvCovWWs
    return Y, CovWW, CovWWs, CovWWp, CovC11, CovC12, CovC21, CovC22


def conditional_ite_vec(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, d):
    """src/estimation.jl:36-50 on likelihood_distribution_vec."""
    Y, CovWW, CovWWs, CovWWp, C11, C12, C21, C22 = likelihood_distribution_vec(
        uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, d)
    MeanITE = (CovWWs.T - CovWW) @ orc._sym_solve(CovWWp, Y)
    CovITE = C11 - C12 - C21 + C22
    return MeanITE, CovITE


def ite_distributions_vec(samples, X, T, Y, d, pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """src/estimation.jl:66-86 for one intervention vector."""
    n = np.asarray(Y).shape[0]
    S = len(samples)
    MeanITEs = np.zeros((S, n))
    CovITEs = np.zeros((S, n, n))
    for idx, p in enumerate(samples):
        m, C = conditional_ite_vec(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, d)
        MeanITEs[idx] = m
        CovITEs[idx] = orc._symmetric_upper(C) + np.eye(n) * pred_noise
    return MeanITEs, CovITEs


def expected_vec(case, D, samples=None, pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """Restatement outputs for every (sample, level) of the (L, n) levels D; `samples` restricts to those sample indices
    (the arrays keep the call's sample axis, other samples stay zero)."""
    from cases import samples_of
    smp = samples_of(case)
    S, n = case["S"], case["n"]
    D = np.atleast_2d(np.asarray(D, dtype=np.float64))
    L = D.shape[0]
    idx = list(range(S)) if samples is None else list(samples)
    meanITE = np.zeros((n, S, L))
    covITE = np.zeros((S, L, n, n))
    mS = np.zeros((S, L))
    vS = np.zeros((S, L))
    for l in range(L):
        M, Cv = ite_distributions_vec([smp[s] for s in idx], case["X"], case["T"], case["Y"], D[l], pred_noise)
        for k, s in enumerate(idx):
            meanITE[:, s, l] = M[k]
            covITE[s, l] = Cv[k]
            mS[s, l], vS[s, l] = orc.conditional_sate(M[k], Cv[k])
    return dict(meanITE=meanITE, covITE=covITE, meanSATE=mS, varSATE=vS)


def policy(case, L, seed=0):
    """L intervention vectors (L, n) of the kinds causal questions ask for: a shift T + c, or "change a random half, leave
    the rest as observed" — 0 / 1 valued for binary treatments."""
    rng = np.random.default_rng(1000 + seed)
    T = case["T"]
    n = T.shape[0]
    out = np.empty((L, n))
    for l in range(L):
        keep = rng.random(n) < 0.5
        if case["binary_t"]:
            out[l] = np.where(keep, T, float(l % 2))
        elif l % 3 == 0:
            out[l] = T + 0.5 * (1 + l / max(L, 1))
        else:
            out[l] = np.where(keep, T, rng.standard_normal(n))
    return out


def mixed(case, seed=0):
    """d_i = T_i on a random half of the individuals (the policy leaves them as observed), another value elsewhere."""
    rng = np.random.default_rng(2000 + seed)
    T = case["T"]
    keep = rng.random(T.shape[0]) < 0.5
    other = 1.0 - T if case["binary_t"] else T + 0.75
    return np.where(keep, T, other), keep
