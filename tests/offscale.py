"""Inputs off the unit scale (test infrastructure): transforms of a `cases.make_case` dictionary that the RBF model must not
notice — a change of a column's unit, of the outcome's unit, of the origin — plus the cases, the exponential's argument ladder
and the numpy emulation of the mixed-precision mode that tests/test_offscale_reference.py (CPU) and tests/test_gpu_offscale.py
(GPU) share.  Every transform returns a NEW dictionary.  Besides `doTs` a case may carry `sweep` (a longer run of scalar levels),
`baseline` (one value per level of `doTs`) and `levels` (an (L, n) array of per-individual interventions): whatever is there is
transformed like T."""
import numpy as np

import cases

LEVEL_KEYS = ("doTs", "sweep", "baseline", "levels")


def _copy(case):
    return {k: (np.array(v, copy=True, order="K") if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def _each_level_key(c, fn):
    for k in LEVEL_KEYS:
        if c.get(k) is not None:
            c[k] = fn(np.asarray(c[k], dtype=np.float64))


def rescale_features(case, eX, eU, eT):
    """Column k of X and xyLS[k, :] times 2**eX[k], likewise U / uyLS with eU, and T, tyLS and every level times 2**eT: powers
    of two, so x * (1 / ls), d * d * wt and 1 / (tl * tl) keep every bit."""
    c = _copy(case)
    if c["X"] is not None:
        f = np.ldexp(1.0, np.asarray(eX, dtype=np.int64))
        c["X"] = c["X"] * f[None, :]
        c["xyLS"] = np.asfortranarray(c["xyLS"] * f[:, None])
    if c["U"] is not None:
        f = np.ldexp(1.0, np.asarray(eU, dtype=np.int64))
        c["U"] = np.asfortranarray(c["U"] * f[None, :, None])
        c["uyLS"] = np.asfortranarray(c["uyLS"] * f[:, None])
    ft = float(np.ldexp(1.0, int(eT)))
    c["T"] = c["T"] * ft
    c["tyLS"] = c["tyLS"] * ft
    _each_level_key(c, lambda a: a * ft)
    return c


def rescale_outcome(case, k):
    """Y times 2**k, yScale and yNoise times 4**k (the caller multiplies predictionCovarianceNoise by 4**k): A becomes 4**k A,
    its factor 2**k L, and every output a power of two times what it was."""
    c = _copy(case)
    c["Y"] = c["Y"] * float(np.ldexp(1.0, k))
    c["yScale"] = c["yScale"] * float(np.ldexp(1.0, 2 * k))
    c["yNoise"] = c["yNoise"] * float(np.ldexp(1.0, 2 * k))
    return c


def shift(case, cX, cU, cT):
    """Per-column constants added to X and U (every posterior sample's U alike), cT to T and to every level."""
    c = _copy(case)
    if c["X"] is not None:
        c["X"] = c["X"] + np.asarray(cX, dtype=np.float64)[None, :]
    if c["U"] is not None:
        c["U"] = np.asfortranarray(c["U"] + np.asarray(cU, dtype=np.float64)[None, :, None])
    c["T"] = c["T"] + float(cT)
    _each_level_key(c, lambda a: a + float(cT))
    return c


def quantise(case, bits=12):
    """X, U, T and the levels rounded to multiples of 2**-bits: adding a power of two up to 2**(52 - bits) / max|x| is then exact
    in fp64, and so is every difference of two shifted values."""
    q = float(np.ldexp(1.0, bits))
    c = _copy(case)
    for k in ("X", "U", "T"):
        if c[k] is not None:
            c[k] = np.asfortranarray(np.round(c[k] * q) / q) if c[k].ndim == 3 else np.round(c[k] * q) / q
    _each_level_key(c, lambda a: np.round(a * q) / q)
    return c


def bits_equal(a, b):
    """Same shape and the same 64 bits in every element: a sign of zero or a NaN cannot hide as behind `==`."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def bits_differ(a, b):
    """How many elements differ in a bit and the largest difference, for an assertion's message."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return f"shapes {a.shape} != {b.shape}"
    bad = a.view(np.uint64) != b.view(np.uint64)
    return f"{int(bad.sum())} of {bad.size} elements differ, max |a - b| = {float(np.max(np.abs(a - b)[bad])) if bad.any() else 0.0:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# The shifted cases (fp64, against the oracle): four model shapes x both treatment types at n = 129 (one live row in a second
# tile) and 200 (two ragged tiles), S = 3.  The constants differ in sign and size between the columns; a binary T stays {0, 1}.
# ---------------------------------------------------------------------------------------------------------------------------
SHIFT_X = (1000.0, -730.5, 12.25)
SHIFT_U = (-1000.0, 350.75)
SHIFT_T = 1000.0
SHIFT_CASES = [(129 if (i + bt) % 2 == 0 else 200, shape, bool(bt))
               for i, shape in enumerate(("UX", "U", "X", "T")) for bt in (0, 1)]


def shift_case_pair(n, shape, bt):
    """(plain, shifted) for one entry of SHIFT_CASES."""
    c = cases.make_case(n, shape, bt, S=3, seed=800 + n + 7 * list(cases.SHAPES).index(shape) + bt)
    return c, shift(c, SHIFT_X, SHIFT_U, 0.0 if bt else SHIFT_T)


# ---------------------------------------------------------------------------------------------------------------------------
# The mixed-precision mode (GPSLC_FLAG_FP32_KERNEL) as numpy: the operations of gram_kernel<float> and ite_mean_kernel<float> in
# their order.  Features are staged as fp32((x [- x_0]) * (1 / ls)), T as fp32(T [- T_0]); differences, their squares summed by
# fma in feature order, expf and yScale * exp in fp32; K = B .* E, the factorisation, the level sums and alpha in fp64.
# centred=False is the arithmetic before features were centred, level differences fp32(T) - fp32(doT); centred=True subtracts
# each column's first element in fp64 before the conversion and rounds the level difference once.  rt=np.float64 is the fp64 path
# (never centred).
# ---------------------------------------------------------------------------------------------------------------------------
def _fma32(d, acc):
    # d, acc fp32: d * d is exact in fp64 (48 bits), one rounding of the sum to fp64 and one to fp32
    return (d.astype(np.float64) * d.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def emulate_kernel_mode(case, rt=np.float32, centred=True):
    """(meanSATE (S, L), MeanITE (n, S, L)) of `predict` as the kernels of the `rt` arithmetic compute them."""
    n, S = case["n"], case["S"]
    T, Y = case["T"], case["Y"]
    doTs = np.asarray(case["doTs"], dtype=np.float64)
    f32 = rt == np.float32
    cen = f32 and centred
    ms = np.zeros((S, len(doTs)))
    mi = np.zeros((n, S, len(doTs)))
    for s, p in enumerate(cases.samples_of(case)):
        cols = []
        if p.U is not None:
            cols += [(p.U[:, k], p.uyLS[k]) for k in range(p.U.shape[1])]
        if case["X"] is not None:
            cols += [(case["X"][:, k], p.xyLS[k]) for k in range(case["X"].shape[1])]
        lux = np.zeros((n, n), dtype=rt)
        for x, ls in cols:
            v = ((x - x[0]) if cen else x) * (1.0 / ls)
            v = v.astype(rt)
            d = v[:, None] - v[None, :]
            lux = _fma32(d, lux) if f32 else d * d + lux
        B = (rt(p.yScale) * np.exp(-lux)).astype(rt)
        tv = ((T - T[0]) if cen else T).astype(rt)
        wt = 1.0 / (p.tyLS * p.tyLS)
        dt = tv[:, None] - tv[None, :]
        E = np.exp(-((dt * dt) * rt(wt))).astype(rt)
        Bd = B.astype(np.float64)
        K = Bd * E.astype(np.float64)
        alpha = np.linalg.solve(K + p.yNoise * np.eye(n), Y)
        bsum, ksum = Bd.sum(axis=0), K.sum(axis=0)
        ka = Y - p.yNoise * alpha
        for l, doT in enumerate(doTs):
            r64 = np.exp(-(((T - doT) * (T - doT)) * wt))              # the level sums: fp64 in either mode
            ms[s, l] = ((r64 * bsum - ksum) @ alpha) / n
            dl = (T - doT).astype(rt) if (cen or not f32) else T.astype(rt) - rt(doT)
            r = np.exp(-((dl * dl) * rt(wt))).astype(np.float64)
            mi[:, s, l] = Bd @ (r * alpha) - ka
    return ms, mi


def drift(ms, mi, ref_ms, ref_mi):
    """(meanSATE, MeanITE) drift as test_fp32_kernel_mode_drift_and_identities measures it: max relative, max / max."""
    return (float(np.max(np.abs(ms - ref_ms) / np.abs(ref_ms))),
            float(np.max(np.abs(mi - ref_mi)) / np.max(np.abs(ref_mi))))


FP32_SHIFTS = (0.0, 100.0, 1e4)


def fp32_base_cases():
    """The cases of the mixed-precision budget, name -> case: the n = 300 case of test_fp32_kernel_mode_drift_and_identities at
    L = 2 and at L = 17 (the 16-level VALU path), shape X with nX = 14 (the float runtime-F Gram path) and a binary treatment."""
    main = cases.make_case(300, "UX", False, S=4, seed=21)
    # Y = sin(T) + ...: every sample's effect curve crosses zero near doT = 0 (the oracle's meanSATE is -0.04 .. -0.01 at 0.0),
    # and a RELATIVE bound on meanSATE says nothing at a crossing.  The 17 levels lie on both sides of it, where the oracle's
    # |meanSATE| is 0.07 .. 0.39.
    return {"main_L2": main,
            "main_L17": dict(main, doTs=np.concatenate([np.linspace(-1.5, -0.4, 8), np.linspace(0.4, 1.6, 9)])),
            "X14": cases.make_case(200, "X", False, S=3, nX=14, seed=841),
            "binary": cases.make_case(200, "UX", True, S=3, seed=842)}


def fp32_shifted(case, c):
    """Every column of X and U, T (unless binary) and the levels moved by c."""
    nX = 0 if case["X"] is None else case["X"].shape[1]
    nU = 0 if case["U"] is None else case["U"].shape[1]
    return shift(case, [c] * nX, [c] * nU, 0.0 if case["binary_t"] else c)


# ---------------------------------------------------------------------------------------------------------------------------
# exp over its whole domain: a_j = t_j^2 with tyLS = 1, t_0 = 0.  Around every reduction breakpoint of gp_exp_neg (|x| = ln2 / 2:
# k = rint(x / ln2) steps) and of gp_exp_neg_tab (|x| = ln2 / 64 (2m + 1): k = rint(32 x / ln2) steps; m = 15, 16: the table index
# wraps), the -800 clamp, the results that are subnormal (744.44 < a < 745.13) and zero.
# ---------------------------------------------------------------------------------------------------------------------------
EXP_N = 129


def exp_ladder_t():
    """t (EXP_N,), t[0] = 0: the ladder's t_j, the rest of the array filled with a grid over the subnormal range."""
    ln2 = float(np.log(2.0))
    t = [0.0, 1e-9]                                                  # a = 0, 1e-18
    for bp in [ln2 / 2] + [ln2 / 64 * (2 * m + 1) for m in (0, 1, 2, 3, 15, 16, 31)] + [ln2 * 1.5, ln2 * 1074.5]:
        r = float(np.sqrt(bp))
        t += [float(np.nextafter(r, 0.0)), r, float(np.nextafter(r, np.inf))]
    t += [float(np.sqrt(a)) for a in (1.0, 37.4, 700.0, 708.39, 708.40, 744.4, 745.13, 745.14, 790.0, 800.0, 800.5, 1e4)]
    t += [1e150]
    grid = np.linspace(708.0, 746.0, EXP_N - len(t))                 # normal -> subnormal -> zero, 0.4 apart
    t += [float(np.sqrt(a)) for a in grid]
    assert len(t) == EXP_N
    return np.array(t)


def exp_reference(t, wt=1.0):
    """(a, ref): the argument as the kernels form it in fp64, (d * d) * wt with d = t_0 - t_j, and exp(-a) evaluated in long
    double and rounded to double (subnormals and zero included: the conversion rounds correctly)."""
    d = t[0] - t
    a = (d * d) * wt
    with np.errstate(under="ignore"):
        ref = np.exp(-a.astype(np.longdouble)).astype(np.float64)
    return a, ref


def ulp_distance_bound(ref):
    """One unit in the last place of each reference value (subnormal or zero: the subnormal spacing 2**-1074)."""
    return np.maximum(np.spacing(np.abs(ref)), float(np.ldexp(1.0, -1074)))


def bridged_cases():
    """name -> case: the bridged clusters at L = 2 (the VALU MeanITE kernel) and at L = 9 (the MFMA form; levels on both sides of
    the effect's zero crossing, as fp32_base_cases)."""
    c = bridged_clusters_case()
    return {"L2": c, "L9": dict(c, doTs=np.concatenate([np.linspace(-1.5, -0.4, 4), np.linspace(0.4, 1.6, 5)]))}


def bridged_clusters_case(n=200, seed=860):
    """Shape X, nX = 3, S = 3: column 0 (lengthscale 1) holds two clusters 60 lengthscales apart and a dozen bridge points 24.5
    to 30 from the first — pair exponents -600 .. -900 against it, beyond the -800 clamp against the second: the table-driven
    routine of the Gram build and the MeanITE pass over the part of its domain where the result is subnormal or zero.
    The first cluster is standard normal and holds the column's first element, the mixed-precision mode's centre.  The second is
    0.02 wide: fp32 rounds a value 60 lengthscales from the centre to eps32 * 60 / 2 = 3.6e-6, a pair (d + delta)^2 is off by
    2 d delta, and only |d| << 1 inside that cluster keeps the case inside the mode's 1e-6 budget (the emulation gives a
    MeanITE drift of 3.0e-7 at this width, 1.0e-6 at width 1: tests/test_offscale_reference.py).  That is the price of fp32
    features on data that span 60 lengthscales, not of where the origin is."""
    c = cases.make_case(n, "X", False, S=3, nX=3, seed=seed)
    rng = np.random.Generator(np.random.Philox(seed))
    x = rng.standard_normal(n)
    x[n // 2:] = 60.0 + 0.02 * x[n // 2:]
    x[5:17] = np.linspace(24.5, 30.0, 12)
    c["X"][:, 0] = x
    c["xyLS"][0, :] = 1.0
    return c
