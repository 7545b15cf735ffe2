"""Host restatement of the leave-group-out (LGO) predictive checks of the outcome model Y ~ N(0, A), A = orc.y_cov(...)
(test infrastructure; Rasmussen & Williams §5.4.2 in block form).  Two independent computations per posterior sample:

  closed_form   alpha = inv(A) Y and, per group I, C = inv(A)[I, I] through its Cholesky factor:
                mean_I = Y_I - inv(C) alpha_I, var = diag(inv(C)), lpd = -(m/2) log 2 pi + log det(C)/2 - alpha_I' inv(C) alpha_I / 2;
  refit         literally: delete the group's rows and columns, condition Y_I on the rest, and take the joint Gaussian density
                of Y_I (nobody left: the prior N(0, A)).

Both return (mean (n,), var (n,), lpd (G,)); refit also returns q (G,), the Mahalanobis distance of every group.  Groups are
given as labels in [0, G); a group's members are taken in ascending row order."""
import math

import numpy as np

from loo_restatement import cov_of

LOG2PI = math.log(2.0 * math.pi)


def members_of(labels):
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == g) for g in range(int(labels.max()) + 1)]


def closed_form(A, Y, labels):
    n = A.shape[0]
    groups = members_of(labels)
    Ai = np.linalg.inv(A)
    alpha = Ai @ Y
    mean, var, lpd = np.empty(n), np.empty(n), np.empty(len(groups))
    conds = np.empty(len(groups))
    for g, I in enumerate(groups):
        C = Ai[np.ix_(I, I)]
        conds[g] = np.linalg.cond(C)
        R = np.linalg.cholesky(C)
        z = np.linalg.solve(R, alpha[I])
        mean[I] = Y[I] - np.linalg.solve(R.T, z)
        Ri = np.linalg.inv(R)
        var[I] = np.sum(Ri * Ri, axis=0)
        lpd[g] = -0.5 * len(I) * LOG2PI + np.sum(np.log(np.diag(R))) - 0.5 * (z @ z)
    return (mean, var, lpd), conds


def refit(A, Y, labels):
    n = A.shape[0]
    groups = members_of(labels)
    mean, var, lpd, q = np.empty(n), np.empty(n), np.empty(len(groups)), np.empty(len(groups))
    for g, I in enumerate(groups):
        keep = np.ones(n, dtype=bool)
        keep[I] = False
        if not keep.any():
            mu, cov = np.zeros(len(I)), A[np.ix_(I, I)]
        else:
            K = A[np.ix_(keep, I)]
            sol = np.linalg.solve(A[np.ix_(keep, keep)], np.column_stack([Y[keep], K]))
            mu = K.T @ sol[:, 0]
            cov = A[np.ix_(I, I)] - K.T @ sol[:, 1:]
            cov = 0.5 * (cov + cov.T)
        L = np.linalg.cholesky(cov)
        r = np.linalg.solve(L, Y[I] - mu)
        q[g] = r @ r
        mean[I], var[I] = mu, np.diag(cov)
        lpd[g] = -0.5 * len(I) * LOG2PI - np.sum(np.log(np.diag(L))) - 0.5 * q[g]
    return (mean, var, lpd), q


def tolerance(A, cond_c):
    """The bound of one sample: max(1e-10, 1e-14 cond(A) max_g cond(C_g)) — the bound of loo_restatement.tolerance for the
    entries of W, times the condition of the block that is then solved with.  Returns (tol, cond(A))."""
    cond = float(np.linalg.cond(A))
    return max(1e-10, 1e-14 * cond * float(np.max(cond_c))), cond


def errors(got, ref, q, Y, labels):
    """(lgoVar relative, lgoMean absolute / max|Y|, lgoLpd absolute / (m_g + q_g)) of got = (mean, var, lpd) against ref; q: the
    refit's Mahalanobis distances.  Each is compared with the sample's `tol`."""
    gm, gv, gl = got
    rm, rv, rl = ref
    m = np.bincount(np.asarray(labels), minlength=len(rl)).astype(np.float64)
    ymax = max(float(np.max(np.abs(Y))), np.finfo(float).tiny)
    with np.errstate(invalid="ignore"):
        ev = float(np.max(np.abs(gv - rv) / rv))
        em = float(np.max(np.abs(gm - rm))) / ymax
        el = float(np.max(np.abs(gl - rl) / (m + q)))
    return tuple(e if np.isfinite(e) else np.inf for e in (ev, em, el))


def expected(case, labels, samples=None, X=None, Y=None):
    """Per posterior sample of `samples` (default: all): dict(A, tol, cond, cond_c, closed, refit, q) on the case's data or the
    overrides, for the grouping `labels`"""
    import cases
    Y = np.asarray(case["Y"] if Y is None else Y, dtype=np.float64)
    smp = cases.samples_of(case)
    out = {}
    for s in (range(case["S"]) if samples is None else samples):
        A = cov_of(case, smp[s], X)
        closed, cond_c = closed_form(A, Y, labels)
        ref, q = refit(A, Y, labels)
        tol, cond = tolerance(A, cond_c)
        out[s] = dict(A=A, tol=tol, cond=cond, cond_c=float(np.max(cond_c)), closed=closed, refit=ref, q=q)
    return out


# ---- the labellings of the tests --------------------------------------------------------------------------------------
def singletons(n):
    return np.arange(n, dtype=np.int32)


def one_group(n):
    return np.zeros(n, dtype=np.int32)


def mod7(n):
    """scattered members across tile rows, sizes not multiples of 16 or 4 (fewer than 7 individuals: compacted)"""
    return np.unique(np.arange(n) % 7, return_inverse=True)[1].astype(np.int32)


def blocks_of(n, size):
    return (np.arange(n) // size).astype(np.int32)


def with_block(n, lo, hi, rest=17):
    """rows lo .. hi - 1 as one group (the last label), the others in contiguous blocks of `rest`"""
    lab = np.empty(n, dtype=np.int64)
    others = np.r_[np.arange(0, lo), np.arange(hi, n)]
    lab[others] = np.arange(len(others)) // rest
    lab[lo:hi] = (lab[others].max() + 1) if len(others) else 0
    return lab.astype(np.int32)


# ---- group sizes and placements (tests/test_lgo_sizes.py, tests/test_gpu_lgo_sizes.py) ---------------------------------------
# lgo_group_kernel picks its layout from the padded size mp = 16 ceil(m / 16): slab width 128, 64, 32, 32, 16, 16, 16, 16 and
# 1, 3, 6, 10, 15, 21, 28, 36 lower blocks of C over four waves for mp = 16 .. 128; its gather starts at the tile row k0 of the
# group's first member and a member contributes zeros before its own tile row.
SIZES_N = 640                                               # five tiles
SIZES = (33, 48, 49, 80, 81, 96, 97, 112, 44)               # mp = 48, 48, 64, 80, 96, 96, 112, 112, 48; sums to 640
LATE_SIZES = (33, 48, 80, 96, 112, 15)                      # rows 256..639: mp = 48, 48, 80, 96, 112, 16
LATER_SIZES = (128, 113, 64, 50, 32, 31, 17, 16, 61)        # rows 128..639: mp = 128, 128, 64, 64, 32, 32, 32, 16, 64
EDGE_N = 300                                                # three tiles
EDGE_SIZES = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128)


def padded(m):
    return 16 * ((m + 15) // 16)


def _dealt(rows, sizes, first_label):
    """labels for `rows` (already in the order they are dealt): the first sizes[0] get first_label, the next sizes[1] the next"""
    assert sum(sizes) == len(rows)
    return np.repeat(first_label + np.arange(len(sizes)), sizes)


def size_labellings():
    """name -> labels (SIZES_N,), every label in use.
    contiguous: one group of each of SIZES in row order (first members in tile rows 0, 0, 0, 1, 1, 2, 3, 3, 4; several
                straddle a tile boundary);
    scattered:  the same sizes dealt through a fixed permutation of the rows (every group has members in all five tile rows);
    late:       rows 0..255 in blocks of 17, rows 256..639 permuted into groups of LATE_SIZES (first member in tile row 2,
                members scattered over tile rows 2..4);
    later:      rows 0..127 in blocks of 17, rows 128..639 permuted into groups of LATER_SIZES (first member in tile row 1,
                members in tile rows 1..4): with `late`, every mp from 16 to 128 with k0 > 0 and three tile rows or more."""
    n = SIZES_N
    out = {"contiguous": _dealt(np.arange(n), SIZES, 0)}
    lab = np.empty(n, dtype=np.int64)
    lab[np.random.default_rng(640).permutation(n)] = out["contiguous"]
    out["scattered"] = lab
    for name, lo, sizes, seed in (("late", 256, LATE_SIZES, 641), ("later", 128, LATER_SIZES, 642)):
        lab = np.empty(n, dtype=np.int64)
        lab[:lo] = np.arange(lo) // 17
        lab[lo + np.random.default_rng(seed).permutation(n - lo)] = _dealt(np.arange(n - lo), sizes, lab[lo - 1] + 1)
        out[name] = lab
    return {k: v.astype(np.int32) for k, v in out.items()}


def edge_group(m, n=EDGE_N):
    """rows of the one group of m members of the size-edge cases: a fixed permutation of the rows that begins with one row of
    every tile row, so m >= 3 members are scattered over all of them; ascending"""
    perm = np.random.default_rng(300).permutation(n)
    firsts = [int(perm[np.argmax(perm // 128 == t)]) for t in range((n + 127) // 128)]
    order = firsts + [int(p) for p in perm if p not in firsts]
    return np.sort(np.array(order[:m]))


def beside(n, rows, rest):
    """`rows` as group 0, everybody else in row order in blocks of `rest` (1: singletons) with the labels 1, 2, ..."""
    lab = np.zeros(n, dtype=np.int64)
    others = np.setdiff1d(np.arange(n), rows)
    lab[others] = 1 + np.arange(len(others)) // rest
    return lab.astype(np.int32)


def tile_rows(labels):
    """per group: the sorted tile rows its members fall in (the first one is the kernel's k0)"""
    return [sorted(set((I // 128).tolist())) for I in members_of(labels)]
