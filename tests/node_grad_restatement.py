"""Host restatement of the gradient of a Gaussian-process node's score log N(target; 0, A), A = K + noise I,
K_rc = scale exp(-sum_f ((F_rf - F_cf) / ls_f)^2) over the node's own nF feature columns (test infrastructure; DESIGN.md §23,
Rasmussen & Williams §5.4.1).  A node with nF = 0 has K = scale 11'.  With alpha = inv(A) target, Q = alpha alpha' - inv(A),
P = Q o K, c = diag(inv(A)), D_rcf = F_rf - F_cf:

    dF_rf = -2 sum_c P_rc D_rcf / ls_f^2   (EVERY column)         dls_f = sum_rc P_rc D_rcf^2 / ls_f^3
    dnoise = (alpha.alpha - sum c) / 2      dscale = (alpha.target - n - noise (alpha.alpha - sum c)) / (2 scale)      dtarget = -alpha

in fp64 or np.longdouble (grad_restatement.py's kernel and hand-written inverse).  Beside every output its ERROR SCALE, §21's: the
same sum with |alpha_r||alpha_c| + sqrt(c_r c_c) in place of Q and |D| in place of D; (alpha.alpha + sum c) / 2 for dnoise,
(|alpha|.|target| + n + noise (alpha.alpha + sum c)) / (2 scale) for dscale, max|alpha| for dtarget.  A computed output is compared
with tol * scale, tol = max(1e-10, 1e-14 cond(A)).

`gradient(..., block=b, no_transpose=True)` and `gradient(..., block=b, no_mask=True)` restate two mistakes of an implementation
that works on b x b blocks of the lower triangle (b = 16: the single-launch kernel's packed blocks; b = 128: the tiles): leaving
out the blocks above the diagonal — row r then misses every partner in a later block —, and letting the padding of the last block
take part: inv(A) is padded with the identity and alpha, the features and the target with zeros."""
import functools

import numpy as np

from grad_restatement import inverse, kernel, tolerance  # noqa: F401  (tolerance: the callers' bound)

OUTPUTS = ("dF", "dls", "dscale", "dnoise", "dtarget")


def _features(F, ls, n):
    """(F (n, nF), ls (nF,)) of a node's (F or None, ls or None); long-double arrays keep their precision"""
    if F is None or np.size(F) == 0:
        return np.zeros((n, 0)), np.zeros(0)
    F, ls = np.asarray(F), np.asarray(ls).reshape(-1)
    F = F if F.dtype == np.longdouble else F.astype(np.float64)
    ls = ls if ls.dtype == np.longdouble else ls.astype(np.float64)
    return (F[:, None] if F.ndim == 1 else F), ls


def logpdf(node, dt=np.longdouble):
    """log N(target; 0, A) of the node (F, ls, scale, noise, target) from a hand-written factor in precision dt"""
    F, ls, scale, noise, target = node
    n = len(target)
    F, ls = _features(F, ls, n)
    target = np.asarray(target).astype(dt)
    A = kernel(F, ls, scale, dt) + dt(noise) * np.eye(n, dtype=dt)
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    z = np.zeros(n, dt)
    for i in range(n):
        z[i] = (target[i] - L[i, :i] @ z[:i]) / L[i, i]
    return -(z @ z) / 2 - np.log(np.diag(L)).sum() - dt(n) * np.log(2 * dt(np.pi)) / 2


def gradient(node, dt=np.float64, block=16, no_transpose=False, no_mask=False):
    """-> (grads, scales): dicts over OUTPUTS (dF (n, nF), dls (nF,), dscale, dnoise, dtarget (n,)) in precision dt"""
    F, ls, scale, noise, target = node
    n = len(target)
    F, ls = _features(F, ls, n)
    nF = F.shape[1]
    F, ls, Y, ys, yn = F.astype(dt), ls.astype(dt), np.asarray(target).astype(dt), dt(scale), dt(noise)
    K = kernel(F, ls, ys, dt)
    Ai = inverse(K + yn * np.eye(n, dtype=dt))
    al, c = Ai @ Y, np.diag(Ai).copy()
    m = n
    if no_mask:          # the padding of the last block takes part
        m = -(-n // block) * block
        F = np.concatenate([F, np.zeros((m - n, nF), dt)])
        K = kernel(F, ls, ys, dt)
        Aip = np.eye(m, dtype=dt)
        Aip[:n, :n] = Ai
        Ai = Aip
        al, c, Y = np.concatenate([al, np.zeros(m - n, dt)]), np.diag(Ai).copy(), np.concatenate([Y, np.zeros(m - n, dt)])
    P = (np.outer(al, al) - Ai) * K
    Pa = (np.outer(abs(al), abs(al)) + np.sqrt(np.outer(c, c))) * K
    D = F[:, None, :] - F[None, :, :]
    dls = (P[:, :, None] * D * D).sum((0, 1)) / ls ** 3
    sls = (Pa[:, :, None] * D * D).sum((0, 1)) / ls ** 3
    rows = P
    if no_transpose:     # row r sees the partners of its own and of earlier blocks only
        t = np.arange(m) // block
        rows = P * (t[None, :] <= t[:, None])
    dF = -2 * (rows[:, :, None] * D).sum(1) / ls ** 2
    sF = 2 * (Pa[:, :, None] * abs(D)).sum(1) / ls ** 2
    aa, sc, ay = al @ al, c.sum(), al @ Y
    grads = dict(dF=dF[:n], dls=dls, dscale=(ay - n - yn * (aa - sc)) / (2 * ys), dnoise=(aa - sc) / 2, dtarget=-al[:n])
    scales = dict(dF=sF[:n], dls=sls, dscale=(abs(al) @ abs(Y) + n + yn * (aa + sc)) / (2 * ys), dnoise=(aa + sc) / 2,
                  dtarget=np.full(n, np.max(abs(al[:n]))))
    return grads, scales


def node_tolerance(node):
    """(tol, cond(A)) of the node: tol = max(1e-10, 1e-14 cond(A))"""
    F, ls, scale, noise, target = node
    F, ls = _features(F, ls, len(target))
    return tolerance(F, ls, scale, noise)


def errors(got, ref, scales):
    """{output: max |got - ref| / scale over its elements} (an empty output: 0; None: left out), compared in long double"""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g, r = np.asarray(got[k], dtype=np.longdouble), np.asarray(ref[k], dtype=np.longdouble)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        out[k] = float(np.max(np.abs(g - r) / np.asarray(scales[k], dtype=np.longdouble))) if g.size else 0.0
    return out


def expected(key):
    """(grads, scales, tol, cond) in long double of node `key` = the arguments of random_node — computed once per session"""
    return _expected(*(tuple(key) + (None, 0.0)[len(key) - 3:]))


@functools.lru_cache(maxsize=None)
def _expected(n, nF, seed, fseed, offset):
    node = random_node(n, nF, seed, fseed, offset)
    g, s = gradient(node, np.longdouble)
    tol, cond = node_tolerance(node)
    return g, s, tol, cond


def random_node(n, nF, seed, fseed=None, offset=0.0):
    """(F, ls, scale, noise, target): standard-normal features (+ offset) and target, lengthscales uniform on (1.5, 3),
    scale on (0.5, 2), noise on (0.2, 1.5); F and ls None for nF = 0.  fseed: the feature block is that of
    random_node(n, nF, fseed) — the same array object, so that the nodes of a call share one pointer.  One object per node and
    session, however the arguments are spelled."""
    return _random_node(n, nF, seed, fseed, float(offset))


@functools.lru_cache(maxsize=None)
def _random_node(n, nF, seed, fseed, offset):
    rng = np.random.default_rng((seed, n, nF))
    F = None if nF == 0 else np.asfortranarray(rng.standard_normal((n, nF)) + offset)
    if fseed is not None:
        F = _random_node(n, nF, fseed, None, offset)[0]
    ls = None if nF == 0 else rng.uniform(1.5, 3.0, nF)
    sc, nz = rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.5)
    return (F, ls, float(sc), float(nz), rng.standard_normal(n))
