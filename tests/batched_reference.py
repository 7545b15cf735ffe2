"""oracle.structured_sate / structured_ite for many posterior samples at once (fp64, host CPU only).

The GPU suites that run at bench scale (thousands of posterior samples per call) need the structured restatement for
hundreds of samples; one NumPy call per sample costs seconds each at N = 4096.  This module forms the same quantities in
the same order for a batch of samples with torch's batched CPU linear algebra:

    B = yScale exp(-sum_k (U_k - U_k')^2 / uyLS_k^2 - sum_k (X_k - X_k')^2 / xyLS_k^2),  E = exp(-(T - T')^2 / tyLS^2),
    K = B o E,  A = K + yNoise I = L L',  z = L^-1 Y,  per level: r = exp(-(T - doT)^2 / tyLS^2), c = r o colsum(B) - colsum(K),
    w = L^-1 c,  MeanSATE = w.z / n,  VarSATE = (sum K - 2 r.colsum(B) + sum B - w.w + n eps) / n^2,
    logdet = 2 sum log diag L,  quad = z.z,  MeanITE = (L^-1 D')' z with D = B o (r_j - e_ij).

node_scores and mvn_scores do the same for the Gaussian node scores and prior draws (gpslc_nodes_logpdf / nodes_draw,
gpslc_mvn_logpdf / mvn_draw): K = processCov(rbfKernelLog(F, F, ls), scale, noise) per node, or one covariance scaled per
vector; log N(target; 0, K) and chol(K) target.

tests/test_batched_reference.py pins all of them to the oracle.  Threads are capped at 16 for the duration of a call (never sized
from the machine's CPU count: a shared host grants a process far fewer CPUs than it shows).
"""
import contextlib

import numpy as np
import torch

import gpslc_oracle as orc

MAX_THREADS = 16
CHUNK_BYTES = 512 << 20          # one n x n x chunk working array stays below this


@contextlib.contextmanager
def _threads():
    old = torch.get_num_threads()
    torch.set_num_threads(min(old, MAX_THREADS))
    try:
        yield
    finally:
        torch.set_num_threads(old)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _col(a, s):
    """column s of a (k, S) hyperparameter array as a (k,) vector (a (S,) array gives a scalar vector)"""
    a = np.asarray(a, dtype=np.float64)
    return a[..., s] if a.ndim > 1 else np.atleast_1d(a[s])


def structured_batch(X, T, Y, post, samples, doTs, ite_samples=(), pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """The structured restatement for the posterior samples `samples` of `post` (dict: U (n, nU, S) | None, uyLS (nU, S) | None,
    xyLS (nX, S) | None, tyLS, yNoise, yScale (S,) — the layout of synth.make_posterior and cases.make_case) at the levels doTs.

    Returns dict(meanSATE (m, L), varSATE (m, L), logdet (m,), quad (m,), logpdf (m,), meanITE {s: (n, L)}) in the order of
    `samples`; meanITE holds the samples listed in ite_samples (a subset of samples)."""
    samples = [int(s) for s in samples]
    ite_set = set(int(s) for s in ite_samples)
    assert ite_set <= set(samples), "ite_samples must be a subset of samples"
    doTs = np.atleast_1d(np.asarray(doTs, dtype=np.float64))
    Yn = np.asarray(Y, dtype=np.float64)
    n, L = Yn.shape[0], doTs.shape[0]
    m = len(samples)
    out = dict(meanSATE=np.zeros((m, L)), varSATE=np.zeros((m, L)), logdet=np.zeros(m), quad=np.zeros(m),
               logpdf=np.zeros(m), meanITE={})
    U, Xa = post.get("U"), X
    Tt = _t(orc._as_2d(T)[:, 0])
    Yt = _t(Yn)
    Xt = _t(orc._as_2d(Xa)) if Xa is not None else None
    dT2 = (Tt[:, None] - Tt[None, :]) ** 2
    Xd = [(Xt[:, k][:, None] - Xt[:, k][None, :]) ** 2 for k in range(Xt.shape[1])] if Xt is not None else []
    chunk = max(1, min(m, CHUNK_BYTES // (8 * n * n)))
    with _threads(), torch.no_grad():
        for c0 in range(0, m, chunk):
            idx = samples[c0:c0 + chunk]
            b = len(idx)
            lux = torch.zeros((b, n, n), dtype=torch.float64)
            if U is not None:
                Ut = _t(np.stack([np.asarray(U)[:, :, s] for s in idx]))                 # (b, n, nU)
                uls = _t(np.stack([_col(post["uyLS"], s) for s in idx]))                  # (b, nU)
                for k in range(Ut.shape[2]):
                    d = Ut[:, :, k][:, :, None] - Ut[:, :, k][:, None, :]
                    lux += d * d / (uls[:, k] ** 2)[:, None, None]
            if Xt is not None:
                xls = _t(np.stack([_col(post["xyLS"], s) for s in idx]))                  # (b, nX)
                for k, dk in enumerate(Xd):
                    lux += dk[None] / (xls[:, k] ** 2)[:, None, None]
            ysc = _t([float(post["yScale"][s]) for s in idx])
            tls = _t([float(post["tyLS"][s]) for s in idx])
            ynz = _t([float(post["yNoise"][s]) for s in idx])
            Bm = ysc[:, None, None] * torch.exp(-lux)
            del lux
            E = torch.exp(-dT2[None] / (tls ** 2)[:, None, None])
            K = Bm * E
            bsum = Bm.sum(dim=1)                                                          # column sums (b, n)
            ksum = K.sum(dim=1)
            A = K.clone()
            A.diagonal(dim1=1, dim2=2).add_(ynz[:, None])
            Lf = torch.linalg.cholesky(A)
            del A
            r = torch.exp(-((Tt[None, None, :] - _t(doTs)[None, :, None]) ** 2) / (tls ** 2)[:, None, None])    # (b, L, n)
            cvec = r * bsum[:, None, :] - ksum[:, None, :]
            rhs = torch.cat([Yt.expand(b, n)[:, :, None], cvec.transpose(1, 2)], dim=2)    # (b, n, 1 + L)
            sol = torch.linalg.solve_triangular(Lf, rhs, upper=False)
            z, w = sol[:, :, 0], sol[:, :, 1:]
            sum_delta = (ksum.sum(dim=1)[:, None] - 2.0 * torch.einsum("bln,bn->bl", r, bsum)) + bsum.sum(dim=1)[:, None]
            ms = torch.einsum("bnl,bn->bl", w, z) / n
            vs = (sum_delta - (w * w).sum(dim=1) + n * pred_noise) / float(n) ** 2
            logdet = 2.0 * torch.log(torch.diagonal(Lf, dim1=1, dim2=2)).sum(dim=1)
            quad = (z * z).sum(dim=1)
            sl = slice(c0, c0 + b)
            out["meanSATE"][sl] = ms.numpy()
            out["varSATE"][sl] = vs.numpy()
            out["logdet"][sl] = logdet.numpy()
            out["quad"][sl] = quad.numpy()
            for j, s in enumerate(idx):
                if s not in ite_set:
                    continue
                mi = np.zeros((n, L))
                for l in range(L):
                    D = Bm[j] * (r[j, l][None, :] - E[j])
                    V = torch.linalg.solve_triangular(Lf[j], D.T.contiguous(), upper=False)
                    mi[:, l] = (V.T @ z[j]).numpy()
                out["meanITE"][s] = mi
            del Bm, E, K, Lf
    out["logpdf"] = -0.5 * (n * np.log(2 * np.pi) + out["logdet"] + out["quad"])
    return out


_L2PI = float(np.log(2 * np.pi))


def node_scores(nodes):
    """For each node (F (n, nF) | None, ls (nF,), scale, noise, target (n,)): K = processCov(rbfKernelLog(F, F, ls), scale,
    noise) (F = None or nF = 0: scale 11' + noise I).  Returns dict(logpdf (m,), draw (n, m) = chol(K) target, info (m,)):
    info is LAPACK's (1-based first failing pivot, 0 = fine); a failing node's logpdf and draw are NaN."""
    m = len(nodes)
    n = int(np.asarray(nodes[0][4]).shape[0])
    out = dict(logpdf=np.full(m, np.nan), draw=np.full((n, m), np.nan), info=np.zeros(m, dtype=np.int64))
    chunk = max(1, min(m, CHUNK_BYTES // (8 * n * n)))
    with _threads(), torch.no_grad():
        for c0 in range(0, m, chunk):
            part = nodes[c0:c0 + chunk]
            b = len(part)
            lk = torch.zeros((b, n, n), dtype=torch.float64)
            for j, (F, ls, _, _, _) in enumerate(part):
                if F is None or np.asarray(F).size == 0:
                    continue
                Ft = _t(orc._as_2d(F))
                lst = _t(np.atleast_1d(ls))
                for k in range(Ft.shape[1]):     # sequential sum over the features, as rbf_kernel_log
                    d = Ft[:, k][:, None] - Ft[:, k][None, :]
                    lk[j] -= d * d / lst[k] ** 2
            sc = _t([float(q[2]) for q in part])
            nz = _t([float(q[3]) for q in part])
            K = sc[:, None, None] * torch.exp(lk)
            del lk
            K.diagonal(dim1=1, dim2=2).add_(nz[:, None])
            Lf, info = torch.linalg.cholesky_ex(K)
            del K
            tg = _t(np.stack([np.asarray(q[4], dtype=np.float64) for q in part], axis=1).T)     # (b, n)
            z = torch.linalg.solve_triangular(Lf, tg[:, :, None], upper=False)[:, :, 0]
            lp = -0.5 * (n * _L2PI + 2.0 * torch.log(torch.diagonal(Lf, dim1=1, dim2=2)).sum(dim=1) + (z * z).sum(dim=1))
            dr = torch.bmm(Lf, tg[:, :, None])[:, :, 0]
            bad = info.numpy() != 0
            sl = slice(c0, c0 + b)
            out["info"][sl] = info.numpy()
            out["logpdf"][sl] = np.where(bad, np.nan, lp.numpy())
            out["draw"][:, sl] = np.where(bad[None, :], np.nan, dr.numpy().T)
    return out


def mvn_scores(cov, X, covscale=None):
    """log N(x_s; 0, c_s cov) and sqrt(c_s) chol(cov) x_s for the columns x_s of X (n, S), c = covscale (S,) or 1.
    Returns dict(logpdf (S,), draw (n, S)); raises numpy's LinAlgError when cov is not positive definite."""
    X = np.asarray(X, dtype=np.float64).reshape(np.shape(X)[0], -1)
    n, S = X.shape
    cs = np.ones(S) if covscale is None else np.array(np.broadcast_to(np.asarray(covscale, dtype=np.float64), (S,)))
    out = dict(logpdf=np.zeros(S), draw=np.zeros((n, S)))
    chunk = max(1, min(S, CHUNK_BYTES // (8 * n)))
    with _threads(), torch.no_grad():
        Lf, info = torch.linalg.cholesky_ex(_t(cov))
        if int(info) != 0:
            raise np.linalg.LinAlgError(f"not positive definite (info = {int(info)})")
        logdet = 2.0 * float(torch.log(torch.diagonal(Lf)).sum())
        for c0 in range(0, S, chunk):
            sl = slice(c0, min(S, c0 + chunk))
            x = _t(X[:, sl])
            c = _t(cs[sl])
            z = torch.linalg.solve_triangular(Lf, x, upper=False)
            out["logpdf"][sl] = (-0.5 * (n * _L2PI + n * torch.log(c) + logdet + (z * z).sum(dim=0) / c)).numpy()
            out["draw"][:, sl] = (torch.sqrt(c)[None, :] * (Lf @ x)).numpy()
    return out
