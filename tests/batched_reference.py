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

ite_pairs and ite_pair_draws do the same for the full ITE covariance of (posterior sample, level) pairs (gpslc_predict's unit B
and C: ITEDistributions, sampleITE, predictCounterfactualEffects): with Q_ij = exp(-(T_i - d_j)^2 / tyLS^2) and
H_ij = exp(-(d_i - d_j)^2 / tyLS^2) for the level's intervention d (a scalar level: Q_ij = r_i, H = 1),
D = B o (Q' - E),  Delta = B o (E - Q - Q' + H),  V = L^-1 D',  MeanITE = V' z,  CovITE = Symmetric(Delta - V'V) + eps I,
and the draws M + chol(CovITE) z.

tests/test_batched_reference.py pins all of them to the oracle.  Threads are capped at 16 for the duration of a call (never sized
from the machine's CPU count: a shared host grants a process far fewer CPUs than it shows).
"""
import contextlib

import numpy as np
import torch

import cases
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


def _level(doTs, l, n):
    """level l of doTs as an (n,) intervention vector: doTs is (L,) scalar levels or (L, n) vectors"""
    d = np.asarray(doTs, dtype=np.float64)
    return np.full(n, float(d[l])) if d.ndim == 1 else np.ascontiguousarray(d[l])


def _ite_chunks(X, T, Y, post, pairs, doTs, pred_noise):
    """Yields (j0, MeanITE (b, n), CovITE + pred_noise I (b, n, n)) for consecutive chunks of `pairs` ((s, l) tuples); the factor
    of A is formed once per sample of a chunk."""
    pairs = [(int(s), int(l)) for s, l in pairs]
    d_all = np.asarray(doTs, dtype=np.float64)
    vec = d_all.ndim == 2
    Yn = np.asarray(Y, dtype=np.float64)
    n = Yn.shape[0]
    U = post.get("U")
    Tt = _t(orc._as_2d(T)[:, 0])
    Yt = _t(Yn)
    Xt = _t(orc._as_2d(X)) if X is not None else None
    dT2 = (Tt[:, None] - Tt[None, :]) ** 2
    chunk = max(1, min(len(pairs), CHUNK_BYTES // (8 * n * n)))
    eye = torch.eye(n, dtype=torch.float64)
    for j0 in range(0, len(pairs), chunk):
        part = pairs[j0:j0 + chunk]
        smp = sorted(set(s for s, _ in part))
        fac = {}
        for s in smp:
            lux = torch.zeros((n, n), dtype=torch.float64)
            if U is not None:
                Us = _t(np.asarray(U)[:, :, s])
                uls = _t(_col(post["uyLS"], s))
                for k in range(Us.shape[1]):
                    d = Us[:, k][:, None] - Us[:, k][None, :]
                    lux += d * d / uls[k] ** 2
            if Xt is not None:
                xls = _t(_col(post["xyLS"], s))
                for k in range(Xt.shape[1]):
                    d = Xt[:, k][:, None] - Xt[:, k][None, :]
                    lux += d * d / xls[k] ** 2
            tls = float(post["tyLS"][s])
            Bm = float(post["yScale"][s]) * torch.exp(-lux)
            E = torch.exp(-dT2 / tls ** 2)
            Lf = torch.linalg.cholesky(Bm * E + float(post["yNoise"][s]) * eye)
            z = torch.linalg.solve_triangular(Lf, Yt[:, None], upper=False)[:, 0]
            fac[s] = (Bm, E, Lf, z, tls)
        b = len(part)
        M = torch.zeros((b, n), dtype=torch.float64)
        Cv = torch.zeros((b, n, n), dtype=torch.float64)
        for j, (s, l) in enumerate(part):
            Bm, E, Lf, z, tls = fac[s]
            if vec:
                dv = _t(d_all[l])
                Q = torch.exp(-((Tt[:, None] - dv[None, :]) ** 2) / tls ** 2)
                H = torch.exp(-((dv[:, None] - dv[None, :]) ** 2) / tls ** 2)
                D = Bm * (Q.T - E)
                Delta = Bm * (E - Q - Q.T + H)
            else:
                r = torch.exp(-((Tt - float(d_all[l])) ** 2) / tls ** 2)
                D = Bm * (r[None, :] - E)
                Delta = Bm * (E - r[:, None] - r[None, :] + 1.0)
            V = torch.linalg.solve_triangular(Lf, D.T.contiguous(), upper=False)
            M[j] = V.T @ z
            C = Delta - V.T @ V
            Cv[j] = torch.triu(C) + torch.triu(C, 1).T          # Symmetric(C): the upper triangle wins (src/estimation.jl:82)
            Cv[j].diagonal().add_(pred_noise)
        yield j0, M, Cv


def ite_pairs(X, T, Y, post, pairs, doTs, pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """MeanITE (m, n) and CovITE + pred_noise I (m, n, n) of the (sample, level) pairs `pairs`, in their order.  doTs: (L,) scalar
    levels or (L, n) intervention vectors; post as for structured_batch."""
    n = np.asarray(Y).shape[0]
    m = len(pairs)
    out = dict(mean=np.zeros((m, n)), cov=np.zeros((m, n, n)))
    with _threads(), torch.no_grad():
        for j0, M, Cv in _ite_chunks(X, T, Y, post, pairs, doTs, pred_noise):
            out["mean"][j0:j0 + M.shape[0]] = M.numpy()
            out["cov"][j0:j0 + M.shape[0]] = Cv.numpy()
    return out


def ite_pair_draws(X, T, Y, post, pairs, doTs, z, pred_noise=orc.PREDICTION_COVARIANCE_NOISE):
    """M + chol(C) z_j for the pairs (C = CovITE + pred_noise I; z: (m, n, spp), one block of normals per pair).  Keeps no
    covariance beyond its chunk.  Returns dict(draws (m, n, spp), lam_min (m,), lam_max (m,)): the extreme eigenvalues of C, for
    cases.draw_bounds."""
    z = np.asarray(z, dtype=np.float64)
    m, n, spp = z.shape
    assert m == len(pairs)
    out = dict(draws=np.zeros((m, n, spp)), lam_min=np.zeros(m), lam_max=np.zeros(m))
    with _threads(), torch.no_grad():
        for j0, M, Cv in _ite_chunks(X, T, Y, post, pairs, doTs, pred_noise):
            b = M.shape[0]
            Lc = torch.linalg.cholesky(Cv)
            out["draws"][j0:j0 + b] = (M[:, :, None] + Lc @ _t(z[j0:j0 + b])).numpy()
            ev = torch.linalg.eigvalsh(Cv)
            out["lam_min"][j0:j0 + b] = ev[:, 0].numpy()
            out["lam_max"][j0:j0 + b] = ev[:, -1].numpy()
    return out


def first_failing_pivot(C):
    """LAPACK dpotrf's info of C (..., n, n): the 1-based first pivot at which the Cholesky factorisation breaks down, 0 when C
    is positive definite."""
    with _threads(), torch.no_grad():
        info = torch.linalg.cholesky_ex(_t(C)).info
    return info.numpy() if info.ndim else int(info)


def schur_pivots(C, p):
    """The Schur pivots of C up to the 1-based pivot p: (pivots 1 .. p-1 of the factorisation, pivot p), which must have
    succeeded before it (the leading (p-1) x (p-1) block positive definite)."""
    with _threads(), torch.no_grad():
        Ct = _t(C)
        if p == 1:
            return np.zeros(0), float(Ct[0, 0])
        Lf = torch.linalg.cholesky(Ct[:p - 1, :p - 1])
        w = torch.linalg.solve_triangular(Lf, Ct[:p - 1, p - 1:p], upper=False)[:, 0]
        return (torch.diagonal(Lf) ** 2).numpy(), float(Ct[p - 1, p - 1] - w @ w)


def draws_match(got, ref, lam_min, lam_max, z, tight=True):
    """Every draw column of one pair (got, ref, z: (n, spp)) within cases.draw_bounds: the tight bound (tight=True; a
    conditioning too poor for it fails) or the conditioning-aware one.  Returns (ok, worst error / bound)."""
    got, ref, z = (np.asarray(a, dtype=np.float64).reshape(np.shape(a)[0], -1) for a in (got, ref, z))
    worst = 0.0
    for d in range(ref.shape[1]):
        bound, tb, _ = cases.draw_bounds(lam_min, lam_max, np.linalg.norm(z[:, d]), np.linalg.norm(ref[:, d]))
        lim = tb if tight else bound
        if lim is None:
            return False, np.inf
        err = np.linalg.norm(got[:, d] - ref[:, d])
        if not np.isfinite(err):
            return False, np.inf
        worst = max(worst, err / lim)
    return worst <= 1.0, worst
