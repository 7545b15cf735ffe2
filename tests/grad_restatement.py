"""Host restatement of the gradient of the outcome log-likelihood log N(Y; 0, A), A = K + yNoise I,
K_ij = yScale exp(-sum_f ((w_if - w_jf) / l_f)^2), w = [U | X | T], l = [uyLS; xyLS; tyLS] (test infrastructure; Rasmussen &
Williams §5.4.1).  Dense numpy: inv(A) and, with alpha = inv(A) Y, Q = alpha alpha' - inv(A), P = Q o K,
c = diag(inv(A)), D_ijf = w_if - w_jf,

    dLS_f = sum_ij P_ij D_ijf^2 / l_f^3        dU_if = -2 sum_j P_ij D_ijf / l_f^2   (f < nU)
    dyNoise = (alpha.alpha - sum c) / 2        dyScale = (alpha.Y - n - yNoise (alpha.alpha - sum c)) / (2 yScale)        dY = -alpha

in fp64 (np.linalg.inv) or in np.longdouble (a hand-written Cholesky: numpy's LAPACK calls are fp64 only).  Beside every output
its ERROR SCALE: the same sum with |alpha_i||alpha_j| + sqrt(c_i c_j) in place of Q_ij and |D| in place of D — what the terms of
the sum add up to without cancellation; (alpha.alpha + sum c) / 2 for dyNoise, (|alpha|.|Y| + n + yNoise (alpha.alpha + sum c)) /
(2 yScale) for dyScale, max|alpha| for dY.  A computed output is compared with tol * scale, tol = max(1e-10, 1e-14 cond(A)):
test_gpu_loo.py's bound.

`gradient(..., no_colsum=True)` and `gradient(..., no_mask=True)` restate two mistakes a tiled implementation can make (tiles of
128 individuals, the lower tiles (ti, tj), tj <= ti, only): leaving out the column sums of the off-diagonal tiles — individual i
then misses every partner in a later tile —, and letting the padding of the last tile take part: A^-1 is padded with the identity
and alpha, the features and the off-diagonal of A^-1 with zeros."""
import functools

import numpy as np

TILE = 128
OUTPUTS = ("dU", "duyLS", "dxyLS", "dtyLS", "dyScale", "dyNoise", "dY")


def inputs(case, s, X=None, Y=None):
    """(W (n, F), ls (F,), nU, nX, yScale, yNoise, Y) of posterior sample s of a cases.make_case case"""
    cols, ls = [], []
    nU = 0 if case["U"] is None else case["U"].shape[1]
    X = case["X"] if X is None else X
    nX = 0 if X is None else X.shape[1]
    if nU:
        cols.append(case["U"][:, :, s]); ls.append(case["uyLS"][:, s])
    if nX:
        cols.append(X); ls.append(case["xyLS"][:, s])
    cols.append(case["T"][:, None]); ls.append(case["tyLS"][s:s + 1])
    Y = np.asarray(case["Y"] if Y is None else Y, dtype=np.float64)
    return (np.concatenate(cols, axis=1), np.concatenate(ls), nU, nX, float(case["yScale"][s]), float(case["yNoise"][s]), Y)


def kernel(W, ls, ys, dt=np.float64):
    Z = W.astype(dt) / ls.astype(dt)
    d = Z[:, None, :] - Z[None, :, :]
    return dt(ys) * np.exp(-(d * d).sum(-1))


def cholesky(A):
    """lower factor in A's own precision, column by column"""
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def inverse(A):
    """inv(A) of a symmetric positive definite A: LAPACK in fp64, else inv(L)' inv(L) by forward substitution"""
    if A.dtype == np.float64:
        return np.linalg.inv(A)
    n = len(A)
    L = cholesky(A)
    Li = np.zeros_like(A)
    eye = np.eye(n, dtype=A.dtype)
    for r in range(n):
        Li[r] = (eye[r] - L[r, :r] @ Li[:r]) / L[r, r]
    return Li.T @ Li


def logpdf(W, ls, ys, yn, Y, dt=np.longdouble):
    """log N(Y; 0, A) from the hand-written factor"""
    n = len(Y)
    Y = Y.astype(dt)
    L = cholesky(kernel(W, ls, ys, dt) + dt(yn) * np.eye(n, dtype=dt))
    z = np.zeros(n, dt)
    for i in range(n):
        z[i] = (Y[i] - L[i, :i] @ z[:i]) / L[i, i]
    return -(z @ z) / 2 - np.log(np.diag(L)).sum() - dt(n) * np.log(2 * dt(np.pi)) / 2


def gradient(W, ls, ys, yn, Y, nU, nX, dt=np.float64, no_colsum=False, no_mask=False):
    """-> (grads, scales): dicts over OUTPUTS (dU (n, nU), duyLS (nU,), dxyLS (nX,), scalars, dY (n,)) in precision dt"""
    n, F = W.shape
    W, ls, Y, ys, yn = W.astype(dt), ls.astype(dt), Y.astype(dt), dt(ys), dt(yn)
    K = kernel(W, ls, ys, dt)
    Ai = inverse(K + yn * np.eye(n, dtype=dt))
    al, c = Ai @ Y, np.diag(Ai).copy()
    m = n
    if no_mask:          # the padding of the last tile takes part: identity in A^-1, zeros in alpha, Y and the features
        m = -(-n // TILE) * TILE
        W = np.concatenate([W, np.zeros((m - n, F), dt)])
        K = kernel(W, ls, ys, dt)
        Aip = np.eye(m, dtype=dt)
        Aip[:n, :n] = Ai
        Ai = Aip
        al, c, Y = np.concatenate([al, np.zeros(m - n, dt)]), np.diag(Ai).copy(), np.concatenate([Y, np.zeros(m - n, dt)])
    P = (np.outer(al, al) - Ai) * K
    Pa = (np.outer(abs(al), abs(al)) + np.sqrt(np.outer(c, c))) * K
    D = W[:, None, :] - W[None, :, :]
    dls = (P[:, :, None] * D * D).sum((0, 1)) / ls ** 3
    sls = (Pa[:, :, None] * D * D).sum((0, 1)) / ls ** 3
    rows = P
    if no_colsum:        # individual i sees the partners of its own and of earlier tiles only
        t = np.arange(m) // TILE
        rows = P * (t[None, :] <= t[:, None])
    dU = -2 * (rows[:, :, None] * D[:, :, :nU]).sum(1) / ls[:nU] ** 2
    sU = 2 * (Pa[:, :, None] * abs(D[:, :, :nU])).sum(1) / ls[:nU] ** 2
    aa, sc, ay = al @ al, c.sum(), al @ Y
    grads = dict(dU=dU[:n], duyLS=dls[:nU], dxyLS=dls[nU:nU + nX], dtyLS=dls[F - 1], dyScale=(ay - n - yn * (aa - sc)) / (2 * ys),
                 dyNoise=(aa - sc) / 2, dY=-al[:n])
    scales = dict(dU=sU[:n], duyLS=sls[:nU], dxyLS=sls[nU:nU + nX], dtyLS=sls[F - 1],
                  dyScale=(abs(al) @ abs(Y) + n + yn * (aa + sc)) / (2 * ys), dyNoise=(aa + sc) / 2,
                  dY=np.full(n, np.max(abs(al[:n]))))
    return grads, scales


def tolerance(W, ls, ys, yn):
    """(tol, cond(A)) — loo_restatement.tolerance's bound"""
    cond = float(np.linalg.cond(kernel(W, ls, ys) + yn * np.eye(len(W))))
    return max(1e-10, 1e-14 * cond), cond


def errors(got, ref, scales):
    """{output: max |got - ref| / scale over its elements} (an empty output: 0); the comparison is made in long double"""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g, r = np.asarray(got[k], dtype=np.longdouble), np.asarray(ref[k], dtype=np.longdouble)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        out[k] = float(np.max(np.abs(g - r) / np.asarray(scales[k], dtype=np.longdouble))) if g.size else 0.0
    return out


def expected(case, samples=None, X=None, Y=None, dt=np.longdouble):
    """Per posterior sample of `samples` (default: all): dict(grads, scales, tol, cond) on the case's data or the overrides"""
    out = {}
    for s in (range(case["S"]) if samples is None else samples):
        W, ls, nU, nX, ys, yn, Ys = inputs(case, s, X, Y)
        grads, scales = gradient(W, ls, ys, yn, Ys, nU, nX, dt)
        tol, cond = tolerance(W, ls, ys, yn)
        out[s] = dict(grads=grads, scales=scales, tol=tol, cond=cond)
    return out


def device_sample(out, s):
    """sample s of yLogpdfGrad's / Context.y_logpdf_grad's dict, in `gradient`'s shapes (None stays None)"""
    take = {"dU": lambda a: a[:, :, s], "duyLS": lambda a: a[:, s], "dxyLS": lambda a: a[:, s], "dY": lambda a: a[:, s]}
    return {k: (None if out.get(k) is None else take.get(k, lambda a: a[s])(out[k])) for k in OUTPUTS}


# (n, nU, nX, yNoise, lengthscale range): two tiles with one live row at cond(A) = 182 and 1.8e6, and a model without U at 2.8e3
RANDOM_CASES = ((129, 2, 3, 0.2, (1.5, 3.0)), (129, 2, 3, 1e-5, (3.0, 6.0)), (200, 0, 3, 0.05, (2.0, 4.0)))


@functools.lru_cache(maxsize=None)
def random_inputs(seed=1, cases=RANDOM_CASES):
    """[(W, ls, yScale, yNoise, Y, nU, nX)] of `cases`, drawn one after the other from one generator: standard-normal features and
    outcomes, lengthscales uniform on the case's range, yScale = 1.3"""
    rng = np.random.default_rng(seed)
    out = []
    for n, nU, nX, yn, (lo, hi) in cases:
        F = nU + nX + 1
        W = rng.normal(size=(n, F))
        ls = rng.uniform(lo, hi, F)
        out.append((W, ls, 1.3, yn, rng.normal(size=n), nU, nX))
    return out
