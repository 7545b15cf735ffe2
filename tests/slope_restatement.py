"""Dense NumPy restatement of the estimation path for the marginal effect g_i(a) = d f_i(t) / dt at a scalar level t = a.

The derivative of a Gaussian process is a Gaussian process: differentiating the RBF treatment kernel
k(t, t') = exp(-(t - t')^2 / tyLS^2) of the joint prior of src/likelihood.jl:24-39, with w = 1 / tyLS^2,

    Cov(g_i(a), f_j(T_j))  = B_ij  d/dt  k(t, T_j) at t = a            = B_ij 2 (T_j - a) w k(a, T_j)
    Cov(g_i(a), g_j(a'))   = B_ij  d^2/dt dt'  k(t, t') at (a, a')     = B_ij (2 w - 4 (a - a')^2 w^2) k(a, a')

so, conditioned on Y (src/estimation.jl:36-50 with these blocks),

    D        = CovWWs_a' .* (2 (T_j - a) w)   (column j scaled)
    MeanITE  = D (CovWWp \\ Y)
    CovITE   = 2 w B - D (CovWWp \\ D'),   Symmetric(.) + pred_noise I   (src/estimation.jl:82)

B, CovWWs_a and CovWWp come from the oracle's rbf_kernel_log / process_cov, the solves from LAPACK: this is the literal side
(dense n x n blocks); the library is the structured side.  Also here: the dense cross-level covariance of the
weighted slopes of a sweep, and the library's structured formulas in NumPy.
"""
import numpy as np
from scipy.linalg import solve_triangular

import gpslc_oracle as orc

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


def slope_blocks(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a, a2=None):
    """(CovWWp, D_a, D_a2, Kgg): the observed block with its noise, the cross blocks Cov(g(a), Y) and Cov(g(a2), Y) (rows: the
    individuals whose slope it is) and the prior block Cov(g(a), g(a2)); a2 defaults to a."""
    Y = np.asarray(Y, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    n = Y.shape[0]
    a2 = a if a2 is None else a2
    Tm = orc._as_2d(T)
    base = _base_log(U, uyLS, X, xyLS, n)
    w = 1.0 / (tyLS * tyLS)
    CovWWp = orc.process_cov(base + orc.rbf_kernel_log(Tm, Tm, tyLS), yScale, 0.0) + yNoise * np.eye(n)

    def cross(x):
        xv = np.full((n, 1), float(x))
        CovWWs = orc.process_cov(base + orc.rbf_kernel_log(Tm, xv, tyLS), yScale, 0.0)       # [j, i] = B_ji k(T_j, x)
        return CovWWs.T * (2.0 * (T - float(x)) * w)[None, :]

    av, bv = np.full((n, 1), float(a)), np.full((n, 1), float(a2))
    Kab = orc.process_cov(base + orc.rbf_kernel_log(av, bv, tyLS), yScale, 0.0)              # B k(a, a2)
    d = float(a) - float(a2)
    Kgg = Kab * (2.0 * w - 4.0 * (d * d) * (w * w))
    return CovWWp, cross(a), cross(a2), Kgg


def conditional_ite_slope(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a):
    """MeanITE (n,), CovITE (n, n) of d f / dt at a given Y; no jitter, like src/estimation.jl:36-50."""
    CovWWp, D, _, Kgg = slope_blocks(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, a)
    MeanITE = D @ orc._sym_solve(CovWWp, np.asarray(Y, dtype=np.float64))
    CovITE = Kgg - D @ orc._sym_solve(CovWWp, D.T)
    return MeanITE, CovITE


def ite_distributions_slope(samples, X, T, Y, a, pred_noise=PN):
    """src/estimation.jl:66-86 for the slope at a."""
    n = np.asarray(Y).shape[0]
    S = len(samples)
    MeanITEs = np.zeros((S, n))
    CovITEs = np.zeros((S, n, n))
    for idx, p in enumerate(samples):
        m, C = conditional_ite_slope(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, a)
        MeanITEs[idx] = m
        CovITEs[idx] = orc._symmetric_upper(C) + np.eye(n) * pred_noise
    return MeanITEs, CovITEs


def expected_slope(case, A, samples=None, pred_noise=PN, want_cov=True):
    """Restatement outputs for every (sample, level) of the levels A; `samples` restricts to those sample indices (the arrays
    keep the call's sample axis, other samples stay zero).  want_cov=False drops the (S, L, n, n) array."""
    from cases import samples_of
    smp = samples_of(case)
    S, n = case["S"], case["n"]
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    L = A.shape[0]
    idx = list(range(S)) if samples is None else list(samples)
    meanITE = np.zeros((n, S, L))
    covITE = np.zeros((S, L, n, n)) if want_cov else None
    mS = np.zeros((S, L))
    vS = np.zeros((S, L))
    for l in range(L):
        M, Cv = ite_distributions_slope([smp[s] for s in idx], case["X"], case["T"], case["Y"], A[l], pred_noise)
        for k, s in enumerate(idx):
            meanITE[:, s, l] = M[k]
            if want_cov:
                covITE[s, l] = Cv[k]
            mS[s, l], vS[s, l] = orc.conditional_sate(M[k], Cv[k])
    return dict(meanITE=meanITE, covITE=covITE, meanSATE=mS, varSATE=vS)


def levels(case, L):
    """L scalar levels: for a continuous treatment the case's own two, then a sweep over [-1.5, 1.5]; for a binary one levels
    at and between the two treatment values."""
    if case["binary_t"]:
        return np.array([(0.3, 1.0, 0.0, 0.5, 0.8)[l % 5] + 0.01 * (l // 5) for l in range(L)])
    return np.concatenate([case["doTs"], np.linspace(-1.5, 1.5, max(L - 2, 0))])[:L].copy()


def literal_slope_curve(case, s, doTs, W, pred_noise=PN):
    """Dense mean (L, G) and joint covariance (L, L, G) of tau_l = w_g' g(a_l) for posterior sample s: every (l, l') block
    Cov(g(a_l), g(a_l') | Y) is formed n x n and summed against the weights."""
    from cases import samples_of
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    p = samples_of(case)[s]
    X, T, Y = case["X"], case["T"], np.asarray(case["Y"], dtype=np.float64)
    L, G = doTs.shape[0], W.shape[0]
    mean, cov = np.zeros((L, G)), np.zeros((L, L, G))
    ww = np.sum(W * W, axis=1)
    for l in range(L):
        for lp in range(l + 1):
            CovWWp, Dl, Dlp, Kgg = slope_blocks(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, X, T, Y, doTs[l], doTs[lp])
            Cb = Kgg - Dl @ orc._sym_solve(CovWWp, Dlp.T)
            if l == lp:
                Cb = orc._symmetric_upper(Cb)
                mean[l] = W @ (Dl @ orc._sym_solve(CovWWp, Y))
            v = np.einsum("gi,ij,gj->g", W, Cb, W)
            cov[l, lp] = cov[lp, l] = v + (pred_noise * ww if l == lp else 0.0)
    return mean, cov


def expected_slope_curve(case, doTs, W, pred_noise=PN, samples=None):
    """literal_slope_curve for every sample: mean (S, L, G), cov (S, L, L, G); `samples` restricts (the others stay zero)."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(W)
    S, L, G = case["S"], doTs.shape[0], W.shape[0]
    mean, cov = np.zeros((S, L, G)), np.zeros((S, L, L, G))
    for s in (range(S) if samples is None else samples):
        mean[s], cov[s] = literal_slope_curve(case, s, doTs, W, pred_noise)
    return dict(mean=mean, cov=cov)


def structured_slope_curve(case, s, doTs, w, pred_noise=PN):
    """The library's formulas for one sample and weight vector in NumPy: mean (L,), cov (L, L) of w' g(a_l) — no n x n
    block of the slope is formed: c_l = q^l .* (B w), v_l = L^-1 c_l, P_ll' = (2 w - 4 (a_l - a_l')^2 w^2) rho(a_l, a_l') beta."""
    from cases import samples_of
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    p = samples_of(case)[s]
    n, T, Y = case["n"], np.asarray(case["T"], dtype=np.float64), np.asarray(case["Y"], dtype=np.float64)
    om = 1.0 / (p.tyLS * p.tyLS)
    B = p.yScale * np.exp(_base_log(p.U, p.uyLS, case["X"], p.xyLS, n))
    K = B * np.exp(-((T[:, None] - T[None, :]) ** 2) * om)
    Lc = np.linalg.cholesky(K + p.yNoise * np.eye(n))
    z = solve_triangular(Lc, Y, lower=True)
    bw = B @ w
    beta = float(w @ bw)
    L = doTs.shape[0]
    V = [solve_triangular(Lc, (2.0 * (T - a) * om * np.exp(-((T - a) ** 2) * om)) * bw, lower=True) for a in doTs]
    mean = np.array([float(v @ z) for v in V])
    cov = np.zeros((L, L))
    for l in range(L):
        for lp in range(l + 1):
            d = doTs[l] - doTs[lp]
            P = (2.0 * om - 4.0 * (d * d) * (om * om)) * np.exp(-(d * d) * om) * beta
            cov[l, lp] = cov[lp, l] = (P - float(V[l] @ V[lp])) + (pred_noise * float(w @ w) if l == lp else 0.0)
    return mean, cov


def structured_slope_average(case, s, a, pred_noise=PN):
    """The plain form's formulas: (mean, var) of the 1/n average, mean = w . z / n and
    var = (2 w sum(B) - w . w + n pred_noise) / n^2 with w = L^-1 (q^a .* bsum)."""
    n = case["n"]
    m, c = structured_slope_curve(case, s, [a], np.full(n, 1.0), pred_noise=0.0)
    return m[0] / n, (c[0, 0] + n * pred_noise) / (n * n)


# ---- the finite difference of contrasts the slope is the limit of ---------------------------------------------------
# (n, shape, seed, a): the cases on which tests/test_slope.py measures how far contrast(a + h, a - h) / (2h) is from the slope and
# tests/test_gpu_slope.py compares the library's contrast with the library's slope
FD_CASES = [(129, "UX", 101, 0.4), (200, "X", 102, -0.7), (129, "T", 103, 0.9), (24, "U", 104, 0.1)]


def fd_errors(case, a, h):
    """Per posterior sample, the distance of the central difference of contrasts from the restatement's slope, relative to the
    slope's own size: (MeanITE max-norm, CovITE max-norm, meanSATE, varSATE), no jitter anywhere."""
    import contrast_restatement as cr
    from cases import samples_of
    out = []
    for p in samples_of(case):
        args = (p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, case["X"], case["T"], case["Y"])
        m, C = conditional_ite_slope(*args, a)
        mf, Cf = cr.conditional_ite_contrast(*args, a + h, a - h)
        mf, Cf = mf / (2.0 * h), Cf / (4.0 * h * h)
        ms, vs = orc.conditional_sate(m, orc._symmetric_upper(C))
        msf, vsf = orc.conditional_sate(mf, orc._symmetric_upper(Cf))
        out.append((np.max(np.abs(mf - m)) / np.max(np.abs(m)), np.max(np.abs(Cf - C)) / np.max(np.abs(C)),
                    abs(msf - ms) / abs(ms), abs(vsf - vs) / abs(vs)))
    return np.array(out)


FD_H = 1e-3
# fd_errors(case, a, FD_H), the larger of the two posterior samples, as tests/test_slope.py measured them on the restatement
# (second-order truncation error of the central difference; columns as fd_errors').  test_slope.py checks the record against
# a fresh measurement; test_gpu_slope.py allows the library's own finite difference twice these.
FD_MEASURED = {
    (129, "UX"): (4.675e-06, 1.403e-05, 8.044e-06, 1.450e-05),
    (200, "X"): (8.243e-07, 2.683e-06, 3.306e-07, 3.552e-06),
    (129, "T"): (5.799e-04, 8.101e-06, 5.799e-04, 8.101e-06),
    (24, "U"): (2.550e-06, 7.993e-06, 2.425e-06, 9.672e-06),
}
