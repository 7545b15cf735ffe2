"""Dense NumPy restatement of the predictions for new individuals (gpslc_predict_new): the textbook GP prediction
at inputs that are not in the data, for the three non-factual level forms.

Per posterior sample, with w_j = [u_j | x_j] the features of training individual j and w*_i those of new individual i:

    B_ij   = yScale exp(-sum_f ((w_if - w_jf) / l_f)^2)      K = B .* rho(T_i, T_j)      A = K + yNoise I      alpha = A^-1 Y
    B*_ij  the same between new individual i and training individual j (m x n), B**_ii' between two new ones (m x m)
    rho(x, y) = exp(-(x - y)^2 / tyLS^2),  r^x_j = rho(T_j, x)

and for a level of form   outcome  f*(a):           cross_j = r^a_j                        prior = 1
                          contrast f*(a) - f*(b):   cross_j = r^a_j - r^b_j                prior = 2 (1 - rho(a, b))
                          slope    df*/dt at a:     cross_j = 2 (T_j - a) r^a_j / tyLS^2   prior = 2 / tyLS^2

    D* = B* diag(cross)      mean = D* alpha      cov = prior B** - D* A^-1 D*' + pred_noise I      var = diag(cov)

(the covariance of f(a) at two individuals is B rho(a, a) = B; of the contrast B (rho(a,a) - rho(a,b) - rho(b,a) + rho(b,b)); of
the derivative B d^2 rho(t, t') / dt dt' at t = t' = a, which is 2 B / tyLS^2).

Two sides: `literal` (np.linalg.solve on A, nothing factorised by hand) and `structured` (Cholesky: W* = D* L^-T, var from the
squared row norms — the library's formulas); `structured` also runs in np.longdouble with a Cholesky written out here, the
yardstick tests/test_new_individuals.py measures both against.
"""
import numpy as np
from scipy.linalg import solve_triangular

import gpslc_oracle as orc

PN = orc.PREDICTION_COVARIANCE_NOISE
FORMS = ("outcome", "contrast", "slope")


def new_individuals(case, m, seed=0, copies=()):
    """Features of m new individuals for `case`: Xnew (m, nX) or None, Unew (m, nU, S) or None, drawn like the case's own.
    `copies`: (new index, training index) pairs that become exact copies of that training individual (X and every sample's U)."""
    rng = np.random.Generator(np.random.Philox(977 + seed))
    X, U = case["X"], case["U"]
    Xn = None if X is None else rng.standard_normal((m, X.shape[1]))
    Un = None if U is None else rng.standard_normal((m, U.shape[1], U.shape[2]))
    for i, j in copies:
        if Xn is not None:
            Xn[i] = X[j]
        if Un is not None:
            Un[i] = U[j]
    return (None if Xn is None else np.asfortranarray(Xn)), (None if Un is None else np.asfortranarray(Un))


def _features(case, s, X, U, rows):
    """[U_s | X] / lengthscales, (rows, nU + nX); no columns for a model without features"""
    parts = []
    if case["U"] is not None:
        parts.append(np.asarray(U[:, :, s]) / case["uyLS"][:, s][None, :])
    if case["X"] is not None:
        parts.append(np.asarray(X) / case["xyLS"][:, s][None, :])
    return np.concatenate(parts, axis=1) if parts else np.zeros((rows, 0))


def _rbf(F1, F2, scale, dtype=np.float64):
    d = F1.astype(dtype)[:, None, :] - F2.astype(dtype)[None, :, :]
    return dtype(scale) * np.exp(-np.sum(d * d, axis=2))


def level_factors(form, T, a, b, tyLS, dtype=np.float64):
    """cross (n,), prior of one level"""
    T = np.asarray(T, dtype=dtype)
    a = dtype(a)
    wt = dtype(1.0) / (dtype(tyLS) * dtype(tyLS))
    ra = np.exp(-((T - a) ** 2) * wt)
    if form == "outcome":
        return ra, dtype(1.0)
    if form == "contrast":
        b = dtype(b)
        return ra - np.exp(-((T - b) ** 2) * wt), dtype(2.0) * (dtype(1.0) - np.exp(-((a - b) ** 2) * wt))
    if form == "slope":
        return dtype(2.0) * (T - a) * wt * ra, dtype(2.0) * wt
    raise ValueError(form)


def blocks(case, s, Xn, Un, m, dtype=np.float64):
    """A (n, n), B* (m, n), B** (m, m) of posterior sample s"""
    n = case["n"]
    F, Fn = _features(case, s, case["X"], case["U"], n), _features(case, s, Xn, Un, m)
    ys, T = case["yScale"][s], np.asarray(case["T"], dtype=dtype)
    wt = dtype(1.0) / (dtype(case["tyLS"][s]) ** 2)
    A = _rbf(F, F, ys, dtype) * np.exp(-((T[:, None] - T[None, :]) ** 2) * wt) + dtype(case["yNoise"][s]) * np.eye(n, dtype=dtype)
    return A, _rbf(Fn, F, ys, dtype), _rbf(Fn, Fn, ys, dtype)


def literal(case, s, Xn, Un, m, form, levels, pred_noise=PN, want_cov=True):
    """mean (m, L), var (m, L), cov (L, m, m) or None for `levels` = [(a, b or None), ...] with np.linalg.solve on A"""
    A, Bs, Bss = blocks(case, s, Xn, Un, m)
    alpha = np.linalg.solve(A, np.asarray(case["Y"], dtype=np.float64))
    mean, var = np.zeros((m, len(levels))), np.zeros((m, len(levels)))
    cov = np.zeros((len(levels), m, m)) if want_cov else None
    for l, (a, b) in enumerate(levels):
        cross, prior = level_factors(form, case["T"], a, b, case["tyLS"][s])
        D = Bs * cross[None, :]
        AinvDt = np.linalg.solve(A, D.T)
        mean[:, l] = D @ alpha
        var[:, l] = (prior * np.diag(Bss) - np.sum(D * AinvDt.T, axis=1)) + pred_noise
        if want_cov:
            C = prior * Bss - D @ AinvDt
            cov[l] = 0.5 * (C + C.T) + pred_noise * np.eye(m)
    return mean, var, cov


def _cholesky(A):
    """lower Cholesky factor, column by column in A's own dtype (np.longdouble has no LAPACK)"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for k in range(n):
        c = A[k:, k] - L[k:, :k] @ L[k, :k]
        L[k:, k] = c / np.sqrt(c[0])
    return L


def _forward(L, R):
    """L^-1 R by forward substitution, R (n, q)"""
    out = np.array(R, dtype=L.dtype)
    for k in range(L.shape[0]):
        out[k] = (out[k] - L[k, :k] @ out[:k]) / L[k, k]
    return out


def structured(case, s, Xn, Un, m, form, levels, pred_noise=PN, dtype=np.float64, want_cov=True):
    """The library's formulas for every level of `levels` = [(a, b or None), ...]: mean (m, L), var (m, L), cov (L, m, m) or
    None.  dtype = np.longdouble runs the whole computation (kernel values, Cholesky, solves) in extended precision."""
    A, Bs, Bss = blocks(case, s, Xn, Un, m, dtype)
    Y = np.asarray(case["Y"], dtype=dtype)
    if dtype is np.float64:
        Lc = np.linalg.cholesky(A)
        fwd = lambda R: solve_triangular(Lc, R, lower=True)
    else:
        Lc = _cholesky(A)
        fwd = lambda R: _forward(Lc, R)
    z = fwd(Y[:, None])[:, 0]
    ys = dtype(case["yScale"][s])
    mean = np.zeros((m, len(levels)), dtype=dtype)
    var = np.zeros((m, len(levels)), dtype=dtype)
    cov = np.zeros((len(levels), m, m), dtype=dtype) if want_cov else None
    for l, (a, b) in enumerate(levels):
        cross, prior = level_factors(form, case["T"], a, b, case["tyLS"][s], dtype)
        W = fwd((Bs * cross[None, :]).T).T                       # W* = D* L^-T
        mean[:, l] = W @ z                                         # D* alpha = (D* L^-T)(L^-1 Y)
        var[:, l] = (prior * ys - np.sum(W * W, axis=1)) + dtype(pred_noise)
        if want_cov:
            cov[l] = prior * Bss - W @ W.T + dtype(pred_noise) * np.eye(m, dtype=dtype)
    return mean, var, cov


def pairs(form, L):
    """L levels of a form: [(a, b or None), ...]; contrasts get distinct baselines, level 0 is (0.6, -0.3)"""
    A = np.concatenate([[0.6], np.linspace(-1.5, 1.5, max(L - 1, 0))])[:L]
    if form != "contrast":
        return [(float(a), None) for a in A]
    Bv = np.concatenate([[-0.3], np.linspace(1.1, -0.7, max(L - 1, 0))])[:L]
    return [(float(a), float(b)) for a, b in zip(A, Bv)]


def expected(case, Xn, Un, m, form, levels, pred_noise=PN, want_cov=True, samples=None):
    """The literal side for every (sample, level): mean (m, S, L), var (m, S, L), cov (S, L, m, m) or None; `samples`
    restricts to those sample indices (the others stay zero)."""
    S, L = case["S"], len(levels)
    mean, var = np.zeros((m, S, L)), np.zeros((m, S, L))
    cov = np.zeros((S, L, m, m)) if want_cov else None
    for s in (range(S) if samples is None else samples):
        mu, v, C = literal(case, s, Xn, Un, m, form, levels, pred_noise, want_cov)
        mean[:, s, :], var[:, s, :] = mu, v
        if want_cov:
            cov[s] = C
    return dict(mean=mean, var=var, cov=cov)
