"""Dense NumPy restatement of the weighted averages over new individuals (gpslc_predict_new_weighted): tau_g(l) =
w_g' f*(l) for weight vectors over the m new individuals of tests/new_individuals_restatement.py.

`literal` contracts that module's dense per-individual answer — mean = W mean*, var = w' cov* w with cov* = prior B** - D* A^-1
D*' + pred_noise I from np.linalg.solve on A — and writes the joint covariance of two levels densely,

    Cov(f*_l, f*_l') = joint_ll' B** - D*_l A^-1 D*_l'^T        (m x m, then w' . w),

with joint_ll' the prior covariance of the two level forms at one pair of individuals divided by B**: rho(a, a') for outcomes,
(rho(a, a') - rho(a, b')) - (rho(b, a') - rho(b, b')) for contrasts, d^2 rho(t, t') / dt dt' = (2 / tyLS^2 - 4 (a - a')^2 / tyLS^4)
rho(a, a') for slopes.  `structured` is the library's formulas, which never form an m x m or an m x n product with A^-1:

    bw* = B*' w      beta = w' B** w      c(l) = cross(l) .* bw*      v(l) = L^-1 c(l)      z = L^-1 Y
    mean = v(l) . z      var = (prior_l beta - v(l) . v(l)) + pred_noise (w . w)      cov(l, l') = joint_ll' beta - v(l) . v(l')
"""
import numpy as np
from scipy.linalg import solve_triangular

import new_individuals_restatement as nr

PN = nr.PN
WEIGHT_NAMES = ("everyone", "subgroup", "difference", "unit", "random", "zero")


def weight_set(m, seed=0):
    """The six weight vectors of the tests, (6, m): 1/m (the population average), a subgroup mask's average (every second new
    individual), the difference of that group's and the others' averages (m = 1: the group against itself, zeros), a unit
    vector, random weights of both signs, and a zero column."""
    rng = np.random.default_rng(3000 + seed)
    hi = np.arange(m) % 2 == 0
    lo = ~hi if (~hi).any() else hi
    W = np.zeros((6, m))
    W[0] = 1.0 / m
    W[1] = hi / hi.sum()
    W[2] = hi / hi.sum() - lo / lo.sum()
    W[3, m // 2] = 1.0
    W[4] = rng.standard_normal(m) / m
    return W


def many_weights(m, G, seed=0):
    """G weight vectors (G, m): the six of weight_set, then masks of random subgroups and random signed weights in turn"""
    rng = np.random.default_rng(4000 + seed)
    W = np.zeros((G, m))
    base = weight_set(m, seed)
    for g in range(G):
        if g < 6:
            W[g] = base[g]
        elif g % 2:
            mask = rng.random(m) < 0.3
            mask[int(rng.integers(m))] = True
            W[g] = mask / mask.sum()
        else:
            W[g] = rng.standard_normal(m) / m
    return W


def joint(form, lv, lvp, tyLS):
    """joint_ll' of two levels (a, b or None), (a', b' or None)"""
    wt = 1.0 / (tyLS * tyLS)
    rho = lambda x, y: np.exp(-((x - y) ** 2) * wt)
    (a, b), (ap, bp) = lv, lvp
    if form == "outcome":
        return rho(a, ap)
    if form == "contrast":
        return (rho(a, ap) - rho(a, bp)) - (rho(b, ap) - rho(b, bp))
    if form == "slope":
        return (2.0 * wt - 4.0 * (a - ap) ** 2 * wt * wt) * rho(a, ap)
    raise ValueError(form)


def literal(case, s, Xn, Un, m, form, levels, W, pred_noise=PN, want_cov=True):
    """mean (L, G), var (L, G), cov (L, L, G) or None of sample s for the rows of W (G, m)"""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    L = len(levels)
    mu, _, C = nr.literal(case, s, Xn, Un, m, form, levels, pred_noise)       # (m, L), (L, m, m) with pred_noise I
    mean = (W @ mu).T
    var = np.stack([np.einsum("gi,ij,gj->g", W, C[l], W) for l in range(L)])
    if not want_cov:
        return mean, var, None
    A, Bs, Bss = nr.blocks(case, s, Xn, Un, m)
    D = [Bs * nr.level_factors(form, case["T"], a, b, case["tyLS"][s])[0][None, :] for a, b in levels]
    AinvDt = [np.linalg.solve(A, d.T) for d in D]
    cov = np.zeros((L, L, W.shape[0]))
    for l in range(L):
        for lp in range(L):
            if l == lp:
                cov[l, l] = var[l]
                continue
            Cll = joint(form, levels[l], levels[lp], float(case["tyLS"][s])) * Bss - D[l] @ AinvDt[lp]
            cov[l, lp] = np.einsum("gi,ij,gj->g", W, Cll, W)
    return mean, var, 0.5 * (cov + np.transpose(cov, (1, 0, 2)))


def structured(case, s, Xn, Un, m, form, levels, W, pred_noise=PN):
    """The library's formulas: mean (L, G), var (L, G), cov (L, L, G) of sample s"""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    L, G = len(levels), W.shape[0]
    A, Bs, Bss = nr.blocks(case, s, Xn, Un, m)
    Lc = np.linalg.cholesky(A)
    z = solve_triangular(Lc, np.asarray(case["Y"], dtype=np.float64), lower=True)
    bw = Bs.T @ W.T                                           # (n, G)
    beta = np.einsum("gi,ij,gj->g", W, Bss, W)
    wnorm2 = np.sum(W * W, axis=1)
    tl = float(case["tyLS"][s])
    V, prior = [], []
    for a, b in levels:
        cross, pr = nr.level_factors(form, case["T"], a, b, tl)
        V.append(solve_triangular(Lc, cross[:, None] * bw, lower=True))        # (n, G)
        prior.append(pr)
    mean = np.stack([v.T @ z for v in V])
    var = np.stack([(prior[l] * beta - np.sum(V[l] * V[l], axis=0)) + pred_noise * wnorm2 for l in range(L)])
    cov = np.zeros((L, L, G))
    for l in range(L):
        cov[l, l] = var[l]
        for lp in range(l):        # one value for both triangles, as the library stores it
            cov[l, lp] = cov[lp, l] = joint(form, levels[l], levels[lp], tl) * beta - np.sum(V[l] * V[lp], axis=0)
    return mean, var, cov


def expected(case, Xn, Un, m, form, levels, W, pred_noise=PN, want_cov=True, samples=None):
    """The literal side in the library's shapes: mean (S, L, G), var (S, L, G), cov (S, L, L, G) or None; `samples` restricts
    to those sample indices (the others stay zero)."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    S, L, G = case["S"], len(levels), W.shape[0]
    mean, var = np.zeros((S, L, G)), np.zeros((S, L, G))
    cov = np.zeros((S, L, L, G)) if want_cov else None
    for s in (range(S) if samples is None else samples):
        mu, v, C = literal(case, s, Xn, Un, m, form, levels, W, pred_noise, want_cov)
        mean[s], var[s] = mu, v
        if want_cov:
            cov[s] = C
    return dict(mean=mean, var=var, cov=cov)


def check(got, ref, W, yScale, what, tight=True, worst=None):
    """`got` and `ref`: (mean, var, cov or None) with the sample axis first ((S, L, G), (S, L, L, G)) — every entry inside the
    bounds of weighted_restatement.bounds (required, or tight) with ||w||_1 over the m weights of its column, a covariance entry with the variance
    bound and its own |ref|.  `worst`: a dict that collects the largest error / bound per kind."""
    W = np.atleast_2d(W)
    w1 = np.sum(np.abs(W), axis=1)
    ys = np.asarray(yScale, dtype=np.float64)
    for kind, g_, r_ in zip(("mean", "var", "cov"), got, ref):
        if g_ is None or r_ is None:
            continue
        g_, r_ = np.asarray(g_), np.asarray(r_)
        assert g_.shape == r_.shape, (what, kind, g_.shape, r_.shape)
        sc = ys.reshape((-1,) + (1,) * (r_.ndim - 1))
        if kind == "mean":
            bound = (1e-9 if tight else 1e-6) * np.abs(r_) + (1e-13 if tight else 1e-12) * w1
        else:
            bound = (1e-9 if tight else 1e-6) * np.abs(r_) + (1e-12 if tight else 1e-9) * sc * w1 ** 2
        err = np.abs(g_ - r_)
        if worst is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
            worst[kind] = max(worst.get(kind, 0.0), float(np.max(ratio)))
        assert np.all(err <= bound), (what, kind, float(np.max(err - bound)))
