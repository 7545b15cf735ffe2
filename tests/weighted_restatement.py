"""The literal side of the weighted average effects tau_w = w' ITE.

For a weight vector w over the n individuals, per posterior sample and level,

    mean = w' MeanITE            var = w' (Symmetric(CovITE) + pred_noise I) w

with MeanITE and the dense n x n CovITE from the oracle's own ITEDistributions (oracle/gpslc_oracle.py, the ordinary estimand
f(doT) - f(T)) or from tests/contrast_restatement.py (the contrast f(a) - f(b)).  The library never forms CovITE; this does.
Also the structured formulas of the library in NumPy (`structured`), which tests/test_group_weights.py holds against the
literal side on the CPU, and the weight sets the tests share.
"""
import numpy as np

import contrast_restatement as cr
import gpslc_oracle as orc

PN = orc.PREDICTION_COVARIANCE_NOISE
WEIGHT_NAMES = ("everyone", "treated", "rest", "difference", "unit", "object", "random")


def weight_set(case, seed=0):
    """The seven weight vectors of the tests, (7, n): everyone (1/n: the SATE), the treated (binary T) or the upper half of T,
    the rest, the difference of those two group averages, a unit vector (one individual), one object of 5 consecutive rows
    (cases.make_case groups the rows in objects of 5), and random weights of both signs."""
    n, T = case["n"], case["T"]
    rng = np.random.default_rng(1000 + seed)
    hi = (T == 1.0) if case["binary_t"] else (T > np.median(T))
    if not hi.any() or hi.all():
        hi = np.arange(n) % 2 == 0
    W = np.zeros((7, n))
    W[0] = 1.0 / n
    W[1] = hi / hi.sum()
    W[2] = (~hi) / (~hi).sum()
    W[3] = W[1] - W[2]
    W[4, int(rng.integers(n))] = 1.0
    o = 5 * int(rng.integers((n + 4) // 5))
    W[5, o:o + 5] = 1.0
    W[5] /= W[5].sum()
    W[6] = rng.standard_normal(n) / n
    return W


def many_weights(case, G, seed=0):
    """G weight vectors (G, n): the seven of weight_set, then masks of random subgroups and random signed weights in turn."""
    n = case["n"]
    rng = np.random.default_rng(2000 + seed)
    W = np.zeros((G, n))
    base = weight_set(case, seed)
    for g in range(G):
        if g < 7:
            W[g] = base[g]
        elif g % 2:
            m = rng.random(n) < 0.3
            m[int(rng.integers(n))] = True
            W[g] = m / m.sum()
        else:
            W[g] = rng.standard_normal(n) / n
    return W


def _dists(case, a, b, pred_noise, samples):
    smp = [s_ for k, s_ in enumerate(__import__("cases").samples_of(case)) if k in samples]
    if b is None:
        return orc.ite_distributions(smp, case["X"], case["T"], case["Y"], a, pred_noise)
    return cr.ite_distributions_contrast(smp, case["X"], case["T"], case["Y"], a, b, pred_noise)


def expected_weighted(case, doTs, W, base=None, pred_noise=PN, samples=None):
    """Literal outputs for every (sample, level, weight row): mean (S, L, G), var (S, L, G), and MeanITE (n, S, L).  `base`:
    None = the ordinary estimand, else one baseline per level (the contrast).  `samples` restricts to those sample indices
    (the arrays keep the call's sample axis, other samples stay zero)."""
    S, n = case["S"], case["n"]
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    L, G = doTs.shape[0], W.shape[0]
    idx = list(range(S)) if samples is None else list(samples)
    bs = None if base is None else np.broadcast_to(np.asarray(base, dtype=np.float64), doTs.shape)
    mean, var, mite = np.zeros((S, L, G)), np.zeros((S, L, G)), np.zeros((n, S, L))
    for l in range(L):
        M, Cv = _dists(case, doTs[l], None if bs is None else bs[l], pred_noise, idx)
        for k, s in enumerate(idx):
            mite[:, s, l] = M[k]
            mean[s, l] = W @ M[k]
            var[s, l] = np.einsum("gi,ij,gj->g", W, Cv[k], W)
    return dict(mean=mean, var=var, meanITE=mite)


def structured(case, s, doT, w, base=None, pred_noise=PN):
    """The library's formulas for one sample, level and weight vector, in NumPy: bw = B w, kw = K w, c, w' Delta w,
    v = L^-1 c, mean = v . z, var = (w' Delta w - v . v) + pred_noise (w . w).  Returns (mean, var)."""
    import cases
    p = cases.samples_of(case)[s]
    n, T, Y = case["n"], case["T"], np.asarray(case["Y"], dtype=np.float64)
    lg = np.zeros((n, n))
    if p.U is not None:
        Um = orc._as_2d(p.U)
        lg = lg + orc.rbf_kernel_log(Um, Um, np.atleast_1d(p.uyLS))
    if case["X"] is not None:
        Xm = orc._as_2d(case["X"])
        lg = lg + orc.rbf_kernel_log(Xm, Xm, np.atleast_1d(p.xyLS))
    B = p.yScale * np.exp(lg)
    E = np.exp(-((T[:, None] - T[None, :]) ** 2) / p.tyLS ** 2)
    K = B * E
    Lc = np.linalg.cholesky(K + p.yNoise * np.eye(n))
    from scipy.linalg import solve_triangular
    z = solve_triangular(Lc, Y, lower=True)
    bw, kw = B @ w, K @ w
    r = np.exp(-((T - doT) ** 2) / p.tyLS ** 2)
    if base is None:
        c = r * bw - kw
        wdw = np.sum(w * ((kw - 2.0 * r * bw) + bw))
    else:
        rb = np.exp(-((T - base) ** 2) / p.tyLS ** 2)
        rho = np.exp(-((doT - base) ** 2) / p.tyLS ** 2)
        c = (r - rb) * bw
        wdw = ((1.0 - rho) + (1.0 - rho)) * np.sum(w * bw)
    v = solve_triangular(Lc, c, lower=True)
    return float(v @ z), float((wdw - v @ v) + pred_noise * (w @ w))


def bounds(ref_mean, ref_var, w, yScale):
    """(required mean, required var, tight mean, tight var) error bounds for one weight vector: the project's own
    (tests/test_gpu_contrast.py: _check) scaled with ||w||_1 so that w = 1/n reproduces them exactly."""
    w1 = float(np.sum(np.abs(w)))
    return (1e-6 * abs(ref_mean) + 1e-12 * w1, 1e-6 * abs(ref_var) + 1e-9 * yScale * w1 ** 2,
            1e-9 * abs(ref_mean) + 1e-13 * w1, 1e-9 * abs(ref_var) + 1e-12 * yScale * w1 ** 2)
