"""Dense NumPy restatement of the predictions for new individuals at levels that depend on the individual
(gpslc_predict_new_vec) and of the score of a held-out test set (gpslc_y_test).

Notation of tests/new_individuals_restatement.py (A, alpha, B* (m x n), B** (m x m), rho).  Level l sets new individual i to the dose
a_il, and for a contrast against b_il:

    outcome   f*_i(a_i):               cross_ij = rho(T_j, a_i)                    P_ii' = rho(a_i, a_i')
    contrast  f*_i(a_i) - f*_i(b_i):   cross_ij = rho(T_j, a_i) - rho(T_j, b_i)    P_ii' = rho(a_i,a_i') - rho(a_i,b_i') - rho(b_i,a_i') + rho(b_i,b_i')

    D* = B* .* cross      mean = D* alpha      cov = P .* B** - D* A^-1 D*' + noise I      var = diag(cov)

The test-set score is the outcome form with a_i = Ttest_i and noise = yNoise of the sample: lpd_i = log N(Ytest_i; mean_i, var_i) and
lpd_joint = log N(Ytest; mean, cov).

Three sides as there: `literal` (np.linalg.solve on A; slogdet / solve on cov), `structured` (Cholesky, W* = D* L^-T, row norms — the
library's formulas) in float64, and `structured` in np.longdouble, the yardstick tests/test_new_vec.py measures both against.
"""
import numpy as np
from scipy.linalg import solve_triangular

import new_individuals_restatement as nr

PN = nr.PN
FORMS = ("outcome", "contrast")
LOG2PI = 1.8378770664093454835606594728112353


def doses(m, L, form, seed=0, equal_rows=()):
    """Per-individual doses A (m, L) and, for a contrast, baselines B (m, L), else None; the rows in `equal_rows` get
    b_il = a_il at every level (a contrast of a level with itself)"""
    rng = np.random.Generator(np.random.Philox(4242 + seed))
    A = rng.uniform(-1.5, 1.5, size=(m, L))
    if form != "contrast":
        return np.asfortranarray(A), None
    B = rng.uniform(-1.5, 1.5, size=(m, L))
    for i in equal_rows:
        B[i] = A[i]
    return np.asfortranarray(A), np.asfortranarray(B)


def _rho(x, y, wt):
    return np.exp(-((x[:, None] - y[None, :]) ** 2) * wt)


def level_factors(form, T, a, b, tyLS, dtype=np.float64):
    """cross (m, n) and P (m, m) of one level with doses a (m,) and baselines b (m,) or None"""
    T, a = np.asarray(T, dtype=dtype), np.asarray(a, dtype=dtype)
    wt = dtype(1.0) / (dtype(tyLS) * dtype(tyLS))
    if form == "outcome":
        return _rho(a, T, wt), _rho(a, a, wt)
    if form == "contrast":
        b = np.asarray(b, dtype=dtype)
        return _rho(a, T, wt) - _rho(b, T, wt), (_rho(a, a, wt) - _rho(a, b, wt)) - (_rho(b, a, wt) - _rho(b, b, wt))
    raise ValueError(form)


def literal(case, s, Xn, Un, m, form, A_, B_, noise=PN, want_cov=True):
    """mean (m, L), var (m, L), cov (L, m, m) or None with np.linalg.solve on A"""
    A, Bs, Bss = nr.blocks(case, s, Xn, Un, m)
    alpha = np.linalg.solve(A, np.asarray(case["Y"], dtype=np.float64))
    L = A_.shape[1]
    mean, var = np.zeros((m, L)), np.zeros((m, L))
    cov = np.zeros((L, m, m)) if want_cov else None
    for l in range(L):
        cross, P = level_factors(form, case["T"], A_[:, l], None if B_ is None else B_[:, l], case["tyLS"][s])
        D = Bs * cross
        AinvDt = np.linalg.solve(A, D.T)
        mean[:, l] = D @ alpha
        var[:, l] = (np.diag(P) * np.diag(Bss) - np.sum(D * AinvDt.T, axis=1)) + noise
        if want_cov:
            C = P * Bss - D @ AinvDt
            cov[l] = 0.5 * (C + C.T) + noise * np.eye(m)
    return mean, var, cov


def structured(case, s, Xn, Un, m, form, A_, B_, noise=PN, dtype=np.float64, want_cov=True):
    """The library's formulas: mean (m, L), var (m, L), cov (L, m, m) or None; dtype = np.longdouble runs everything in extended
    precision"""
    A, Bs, Bss = nr.blocks(case, s, Xn, Un, m, dtype)
    Y = np.asarray(case["Y"], dtype=dtype)
    if dtype is np.float64:
        Lc = np.linalg.cholesky(A)
        fwd = lambda R: solve_triangular(Lc, R, lower=True)
    else:
        Lc = nr._cholesky(A)
        fwd = lambda R: nr._forward(Lc, R)
    z = fwd(Y[:, None])[:, 0]
    ys = dtype(case["yScale"][s])
    L = A_.shape[1]
    mean, var = np.zeros((m, L), dtype=dtype), np.zeros((m, L), dtype=dtype)
    cov = np.zeros((L, m, m), dtype=dtype) if want_cov else None
    for l in range(L):
        cross, P = level_factors(form, case["T"], A_[:, l], None if B_ is None else B_[:, l], case["tyLS"][s], dtype)
        W = fwd((Bs * cross).T).T
        mean[:, l] = W @ z
        var[:, l] = (np.diag(P) * ys - np.sum(W * W, axis=1)) + dtype(noise)
        if want_cov:
            cov[l] = P * Bss - W @ W.T + dtype(noise) * np.eye(m, dtype=dtype)
    return mean, var, cov


def expected(case, Xn, Un, m, form, A_, B_, pred_noise=PN, want_cov=True, samples=None):
    """The literal side for every (sample, level): mean (m, S, L), var (m, S, L), cov (S, L, m, m) or None"""
    S, L = case["S"], A_.shape[1]
    mean, var = np.zeros((m, S, L)), np.zeros((m, S, L))
    cov = np.zeros((S, L, m, m)) if want_cov else None
    for s in (range(S) if samples is None else samples):
        mu, v, C = literal(case, s, Xn, Un, m, form, A_, B_, pred_noise, want_cov)
        mean[:, s, :], var[:, s, :] = mu, v
        if want_cov:
            cov[s] = C
    return dict(mean=mean, var=var, cov=cov)


def score(case, s, Xn, Un, m, Tt, Yt, side="literal", dtype=np.float64):
    """mean (m,), var (m,), lpd (m,), lpd_joint and C (m, m) of the test set (Xn, Un, Tt, Yt) under sample s.  `literal`: slogdet
    and solve on C; `structured`: a Cholesky factor of C, its log diagonal and a forward substitution, in `dtype`."""
    Tt = np.asarray(Tt, dtype=np.float64)[:, None]
    noise = case["yNoise"][s]
    if side == "literal":
        mean, var, cov = literal(case, s, Xn, Un, m, "outcome", Tt, None, noise)
    else:
        mean, var, cov = structured(case, s, Xn, Un, m, "outcome", Tt, None, noise, dtype)
    mean, var, C = mean[:, 0], var[:, 0], cov[0]
    r = np.asarray(Yt, dtype=C.dtype) - mean
    half = C.dtype.type(0.5)
    lpd = -half * C.dtype.type(LOG2PI) - half * np.log(var) - half * r * r / var
    if side == "literal":
        sign, logdet = np.linalg.slogdet(C)
        assert sign > 0
        quad = r @ np.linalg.solve(C, r)
    else:
        Lc = np.linalg.cholesky(C) if dtype is np.float64 else nr._cholesky(C)
        logdet = 2 * np.sum(np.log(np.diag(Lc)))
        zr = solve_triangular(Lc, r, lower=True) if dtype is np.float64 else nr._forward(Lc, r[:, None])[:, 0]
        quad = zr @ zr
    return mean, var, lpd, -half * m * C.dtype.type(LOG2PI) - half * logdet - half * quad, C


def expected_score(case, Xn, Un, m, Tt, Yt, samples=None):
    """The literal side for every sample: mean, var, lpd (m, S) and joint (S,)"""
    S = case["S"]
    out = dict(mean=np.zeros((m, S)), var=np.zeros((m, S)), lpd=np.zeros((m, S)), joint=np.zeros(S))
    for s in (range(S) if samples is None else samples):
        out["mean"][:, s], out["var"][:, s], out["lpd"][:, s], out["joint"][s], _ = score(case, s, Xn, Un, m, Tt, Yt)
    return out


def held_out(case, m, seed=0):
    """Treatments and outcomes of m test individuals, drawn like the case's own"""
    rng = np.random.Generator(np.random.Philox(8181 + seed))
    Tt = (rng.random(m) < 0.5).astype(np.float64) if case["binary_t"] else rng.standard_normal(m)
    return Tt, np.sin(Tt) + 0.5 * rng.standard_normal(m)


def pooled(case, Xn, Un, Tt, Yt):
    """The case of the n + m pooled individuals (training rows first): for the chain rule logpdf(pooled) - logpdf(train)"""
    c = dict(case)
    c["n"] = case["n"] + len(Tt)
    c["T"], c["Y"] = np.concatenate([case["T"], Tt]), np.concatenate([case["Y"], Yt])
    c["X"] = None if case["X"] is None else np.concatenate([case["X"], Xn], axis=0)
    c["U"] = None if case["U"] is None else np.asfortranarray(np.concatenate([case["U"], Un], axis=0))
    return c


# ---- the cases tests/test_gpu_new_vec.py runs on the device; tests/test_new_vec.py holds the restatement itself to 1e-3 of the
# device's bounds on every one of them ----------------------------------------------------------------------------------------
# (shape, binary T, n, m, L, form, with cov): n = 24 / 129 / 200 (one tile, one row in the second tile, ragged), m = 1 / 5 / 128 /
# 129 / 300 (mt = 1, 2, 3), L = 1 / 5 with the covariance and L = 9 (two level blocks of the mean kernel) without
GRID = [("UX", False, 24, 5, 5, "outcome", True), ("U", False, 129, 5, 1, "contrast", True), ("X", True, 24, 1, 5, "contrast", True),
        ("T", False, 200, 129, 1, "outcome", True), ("UX", True, 129, 128, 1, "contrast", True), ("X", False, 200, 300, 1, "outcome", True),
        ("U", True, 24, 129, 9, "contrast", False), ("T", True, 129, 5, 9, "outcome", False), ("UX", False, 200, 5, 5, "contrast", True)]
# (shape, binary T, n, m) of the test-set score: mt = 1 (m = 1, 5, 128), 2 (129) and 3 (300)
SCORE_GRID = [("UX", False, 24, 1), ("U", False, 129, 5), ("X", True, 200, 128), ("UX", False, 129, 129), ("X", False, 129, 300),
              ("T", True, 24, 5)]
CHAIN = ("UX", False, 129, 129)      # the chain-rule case: logpdf(n + m pooled) - logpdf(n) = lpd_joint


def grid_case(shape, bt, n, m, L, form):
    """The inputs of one GRID row: case, Xnew, Unew, A (m, L), B (m, L) or None; new individuals 0 and 1 copy training rows n - 1
    and 2, and row 1 of a contrast (m > 1) has b == a at every level"""
    import cases
    c = cases.make_case(n, shape, bt, S=2, seed=17 + n + m + L)
    Xn, Un = nr.new_individuals(c, m, seed=m, copies=[(0, n - 1), (1, 2)][:m])
    A_, B_ = doses(m, L, form, seed=n + m, equal_rows=(1,) if m > 1 else ())
    return c, Xn, Un, A_, B_


def score_case(shape, bt, n, m):
    """The inputs of one SCORE_GRID row: case, Xtest, Utest, Ttest, Ytest"""
    import cases
    c = cases.make_case(n, shape, bt, S=2, seed=23 + n + m)
    Xn, Un = nr.new_individuals(c, m, seed=m + 1)
    return (c, Xn, Un) + held_out(c, m, seed=n + m)
