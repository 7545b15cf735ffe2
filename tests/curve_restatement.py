"""The literal side of the joint covariance of weighted effects across intervention levels.

For levels l = 1..L of one call and a weight vector w, tau_l = w' ITE_l.  The literal side builds the joint Gaussian-process
prior over f at ALL points — the n observed ones (features, T) and, for every level, the n counterfactual ones (the same
features, the treatment replaced by the level; for a contrast two such blocks per level) — block by block from the oracle's
own rbf_kernel_log / process_cov exactly as src/likelihood.jl:24-39 builds its three blocks, conditions on Y, and maps
linearly to the ITEs:

    J_pq    = K_pq - K_p0 (K_00 + yNoise I)^-1 K_0q          posterior covariance of blocks p, q (block 0: the observed points)
    ITE_l   = f_{p(l)} - f_{q(l)}        (p, q) = (level l, 0) ordinary, (a_l, b_l) contrast
    CovITE_ll' = J_pp' - J_pq' - J_qp' + J_qq'
    Cov(tau_l, tau_l') = w' CovITE_ll' w + [l == l'] pred_noise (w . w)            (the jitter of src/estimation.jl:82 is per level)

The library never forms an n x n block; this does.  Also here: the library's structured formulas in NumPy (`structured_curve`)
and the pivoted-Cholesky reference of gpslc_curve_samples.
"""
import numpy as np
from scipy.linalg import solve_triangular

import cases
import contrast_restatement as cr
import gpslc_oracle as orc

PN = orc.PREDICTION_COVARIANCE_NOISE


def curve_levels(c, L, con):
    """L levels (and baselines) of a case; for L >= 4 the last level repeats the first (a rank-deficient block)."""
    if con:
        A, B = cr.pairs(c, L)
        A, B = A.copy(), B.copy()
        if L >= 4:
            A[-1], B[-1] = A[0], B[0]
        return A, B
    lv = np.concatenate([c["doTs"][::-1], np.linspace(-1.1, 1.4, max(L - 2, 0))])[:L].copy()
    if L >= 4:
        lv[-1] = lv[0]
    return lv, None


def _base_log(p, X, n):
    lg = np.zeros((n, n))
    if p.U is not None:
        Um = orc._as_2d(p.U)
        lg = lg + orc.rbf_kernel_log(Um, Um, np.atleast_1d(p.uyLS))
    if X is not None:
        Xm = orc._as_2d(X)
        lg = lg + orc.rbf_kernel_log(Xm, Xm, np.atleast_1d(p.xyLS))
    return lg


class JointGP:
    """The joint prior over the blocks `tvals` (a list of n-vectors of treatment values; block 0 must be the observed T) for
    one posterior sample, conditioned on Y.  Blocks are built on demand: J(p, q) is n x n."""

    def __init__(self, p, X, T, Y, tvals):
        self.p, self.n = p, np.asarray(Y).shape[0]
        self.base = _base_log(p, X, self.n)
        self.t = [orc._as_2d(np.asarray(v, dtype=np.float64)) for v in tvals]
        K00 = self.K(0, 0)
        self.Kyy = K00 + p.yNoise * np.eye(self.n)
        self.A = [self.K(a, 0) for a in range(len(self.t))]                    # K_a0
        self.SA = [orc._sym_solve(self.Kyy, Aa.T) for Aa in self.A]           # Kyy^-1 K_0a
        alpha = orc._sym_solve(self.Kyy, np.asarray(Y, dtype=np.float64))
        self.mean = [Aa @ alpha for Aa in self.A]                             # posterior mean of f at block a

    def K(self, a, b):
        return orc.process_cov(self.base + orc.rbf_kernel_log(self.t[a], self.t[b], self.p.tyLS), self.p.yScale, 0.0)

    def J(self, a, b):
        return self.K(a, b) - self.A[a] @ self.SA[b]


def _blocks(T, doTs, base):
    """(tvals, pairs): the treatment vectors of the joint prior's blocks and, per level, its (p, q) block indices."""
    n = T.shape[0]
    tv = [np.asarray(T, dtype=np.float64)]
    pairs = []
    for l, d in enumerate(doTs):
        tv.append(np.full(n, float(d)))
        if base is None:
            pairs.append((len(tv) - 1, 0))
        else:
            tv.append(np.full(n, float(base[l])))
            pairs.append((len(tv) - 2, len(tv) - 1))
    return tv, pairs


def cov_ite_block(jg, pairs, l, lp):
    """CovITE_ll' (n x n, no jitter, not symmetrised)."""
    (p, q), (pp, qp) = pairs[l], pairs[lp]
    return jg.J(p, pp) - jg.J(p, qp) - jg.J(q, pp) + jg.J(q, qp)


def literal_curve(case, s, doTs, W, base=None, pred_noise=PN):
    """Literal mean (L, G) and joint covariance (L, L, G) of tau_l = w_g' ITE_l for posterior sample s."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    bs = None if base is None else np.broadcast_to(np.asarray(base, dtype=np.float64), doTs.shape)
    p = cases.samples_of(case)[s]
    tv, pairs = _blocks(case["T"], doTs, bs)
    jg = JointGP(p, case["X"], case["T"], case["Y"], tv)
    L, G = doTs.shape[0], W.shape[0]
    mean, cov = np.zeros((L, G)), np.zeros((L, L, G))
    ww = np.sum(W * W, axis=1)
    for l in range(L):
        mean[l] = W @ (jg.mean[pairs[l][0]] - jg.mean[pairs[l][1]])
        for lp in range(l + 1):
            C = cov_ite_block(jg, pairs, l, lp)
            if l == lp:
                C = orc._symmetric_upper(C)
            v = np.einsum("gi,ij,gj->g", W, C, W)
            cov[l, lp] = cov[lp, l] = v + (pred_noise * ww if l == lp else 0.0)
    return mean, cov


def expected_curve(case, doTs, W, base=None, pred_noise=PN, samples=None):
    """literal_curve for every sample: mean (S, L, G), cov (S, L, L, G); `samples` restricts (the others stay zero)."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(W)
    S, L, G = case["S"], doTs.shape[0], W.shape[0]
    mean, cov = np.zeros((S, L, G)), np.zeros((S, L, L, G))
    for s in (range(S) if samples is None else samples):
        mean[s], cov[s] = literal_curve(case, s, doTs, W, base, pred_noise)
    return dict(mean=mean, cov=cov)


def structured_curve(case, s, doTs, w, base=None, pred_noise=PN):
    """The library's formulas for one sample and weight vector in NumPy: mean (L,), cov (L, L)."""
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    p = cases.samples_of(case)[s]
    n, T, Y = case["n"], case["T"], np.asarray(case["Y"], dtype=np.float64)
    B = p.yScale * np.exp(_base_log(p, case["X"], n))
    E = np.exp(-((T[:, None] - T[None, :]) ** 2) / p.tyLS ** 2)
    K = B * E
    Lc = np.linalg.cholesky(K + p.yNoise * np.eye(n))
    z = solve_triangular(Lc, Y, lower=True)
    bw, kw = B @ w, K @ w
    beta, kappa = float(w @ bw), float(w @ kw)
    rho = lambda x, y: np.exp(-((x - y) ** 2) / p.tyLS ** 2)      # noqa: E731
    L = doTs.shape[0]
    r = [rho(T, d) for d in doTs]
    if base is None:
        c = [r[l] * bw - kw for l in range(L)]
        gam = [float(np.sum(w * r[l] * bw)) for l in range(L)]
        P = lambda l, lp: rho(doTs[l], doTs[lp]) * beta - gam[l] - gam[lp] + kappa      # noqa: E731
    else:
        bs = np.broadcast_to(np.asarray(base, dtype=np.float64), doTs.shape)
        c = [(r[l] - rho(T, bs[l])) * bw for l in range(L)]
        P = lambda l, lp: ((rho(doTs[l], doTs[lp]) - rho(doTs[l], bs[lp])) -      # noqa: E731
                           (rho(bs[l], doTs[lp]) - rho(bs[l], bs[lp]))) * beta
    V = [solve_triangular(Lc, cl, lower=True) for cl in c]
    mean = np.array([float(v @ z) for v in V])
    cov = np.zeros((L, L))
    for l in range(L):
        for lp in range(l + 1):
            cov[l, lp] = cov[lp, l] = (P(l, lp) - float(V[l] @ V[lp])) + (pred_noise * float(w @ w) if l == lp else 0.0)
    return mean, cov


def pivoted_factor(C):
    """Diagonally pivoted Cholesky of the symmetric L x L block C (lower triangle read), stopped at the first pivot
    <= L eps max diag: F (L x L, rows in level order, columns in pivot order, zero beyond the rank) with F F' ~ C."""
    C = np.asarray(C, dtype=np.float64)
    Ln = C.shape[0]
    Cs = np.tril(C) + np.tril(C, -1).T
    F = np.zeros((Ln, Ln))
    piv = list(range(Ln))
    dk = np.array([Cs[i, i] for i in range(Ln)])
    stop = Ln * np.finfo(np.float64).eps * max(float(np.max(np.diag(Cs))), 0.0)
    for k in range(Ln):
        m = k + int(np.argmax(dk[k:]))
        if not dk[m] > stop:
            break
        piv[k], piv[m] = piv[m], piv[k]
        dk[k], dk[m] = dk[m], dk[k]
        pk = piv[k]
        lkk = np.sqrt(dk[k])
        F[pk, k] = lkk
        for i in range(k + 1, Ln):
            pi = piv[i]
            v = Cs[pi, pk]
            for j in range(k):
                v -= F[pi, j] * F[pk, j]
            v /= lkk
            F[pi, k] = v
            dk[i] -= v * v
    return F


def curve_samples(mean, cov, spp, z):
    """gpslc_curve_samples with the caller's normals: mean (S, L, G), cov (S, L, L, G), z (L, spp, S, G) -> (L, spp, S, G)."""
    S, L, G = mean.shape
    out = np.zeros((L, spp, S, G))
    for g in range(G):
        for s in range(S):
            F = pivoted_factor(cov[s, :, :, g])
            out[:, :, s, g] = mean[s, :, g][:, None] + F @ z[:, :, s, g]
    return out
