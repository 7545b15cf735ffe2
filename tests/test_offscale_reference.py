"""The reference side of every tolerance tests/test_gpu_offscale.py uses, on the CPU: a failure there cannot be the oracle's own.
  1. On every shifted case (offscale.SHIFT_CASES: X, U and T moved by up to +-1000) the literal, the structured and the 80-bit
     restatements agree as tests/test_oracle_crosscheck.py asks of them on unit-scale data.
  2. The literal restatement of a shifted case agrees with that of the plain case to 1e-11: the oracle does not notice the origin
     (measured at n = 129: 1.1e-13 on CovITE, 4.5e-14 on MeanITE).
  3. The numpy emulation of the mixed-precision mode (offscale.emulate_kernel_mode): rounding x / ls to fp32 before the difference
     breaks the mode's 1e-6 budget at a shift of 100; centring each column on its first element in fp64 first keeps the drift
     below 5e-7 at shifts 0, 100 and 1e4 on exactly the cases the GPU test asserts the budget on.
  4. On every argument of the exponential's ladder the long-double exp, rounded to double, is within one unit in the last place
     of math.exp."""
import math

import numpy as np
import pytest

import cases
import gpslc_oracle as orc
import offscale


@pytest.fixture(scope="module")
def literal():
    """name -> (plain, shifted) oracle_expected, computed once."""
    memo = {}

    def get(n, shape, bt):
        key = (n, shape, bt)
        if key not in memo:
            c, cs = offscale.shift_case_pair(n, shape, bt)
            memo[key] = (c, cs, cases.oracle_expected(c), cases.oracle_expected(cs))
        return memo[key]
    return get


@pytest.mark.parametrize("n,shape,bt", offscale.SHIFT_CASES)
def test_restatements_agree_on_shifted_data(literal, n, shape, bt):
    _, c, _, e = literal(n, shape, bt)
    for s, p in enumerate(cases.samples_of(c)):
        ms, vs, logdet, quad = orc.structured_sate(p, c["X"], c["T"], c["Y"], c["doTs"])
        lp = -0.5 * (n * np.log(2 * np.pi) + logdet + quad)
        assert np.isclose(lp, e["logpdf"][s], rtol=1e-11, atol=1e-9)
        for l, doT in enumerate(c["doTs"]):
            assert abs(ms[l] - e["meanSATE"][s, l]) <= 1e-9 * abs(e["meanSATE"][s, l]) + 1e-13
            assert abs(vs[l] - e["varSATE"][s, l]) <= 1e-9 * abs(e["varSATE"][s, l]) + 1e-12 * p.yScale
            m, cv = orc.structured_ite(p, c["X"], c["T"], c["Y"], doT)
            assert np.max(np.abs(m - e["meanITE"][:, s, l])) <= 1e-9 * np.max(np.abs(e["meanITE"][:, s, l])) + 1e-13
            if s == 0:      # the 80-bit evaluation: one sample per case keeps the CPU suite short
                mld, cld, msld, vsld = orc.literal_sate_longdouble(p, c["X"], c["T"], c["Y"], doT)
                assert abs(float(msld) - e["meanSATE"][s, l]) <= 1e-9 * abs(float(msld)) + 1e-13
                assert abs(float(vsld) - e["varSATE"][s, l]) <= 1e-8 * abs(float(vsld)) + 1e-12 * p.yScale
                assert abs(float(vsld) - vs[l]) <= 1e-8 * abs(float(vsld)) + 1e-12 * p.yScale
                assert np.max(np.abs(cld.astype(float) - e["covITE"][s, l])) <= 1e-9 * p.yScale
                assert np.max(np.abs(mld.astype(float) - e["meanITE"][:, s, l])) <= 1e-9 * np.max(np.abs(e["meanITE"][:, s, l])) + 1e-13


@pytest.mark.parametrize("n,shape,bt", offscale.SHIFT_CASES)
def test_literal_restatement_does_not_notice_the_origin(literal, n, shape, bt):
    c, _, e0, e1 = literal(n, shape, bt)
    worst = {}
    for s in range(c["S"]):
        yS = c["yScale"][s]
        for l in range(len(c["doTs"])):
            m0, m1 = e0["meanITE"][:, s, l], e1["meanITE"][:, s, l]
            worst["MeanITE"] = max(worst.get("MeanITE", 0.0), np.max(np.abs(m1 - m0)) / np.max(np.abs(m0)))
            worst["CovITE"] = max(worst.get("CovITE", 0.0), np.max(np.abs(e1["covITE"][s, l] - e0["covITE"][s, l])) / yS)
            assert np.max(np.abs(m1 - m0)) <= 1e-11 * np.max(np.abs(m0))
            assert np.max(np.abs(e1["covITE"][s, l] - e0["covITE"][s, l])) <= 1e-11 * yS
            assert abs(e1["meanSATE"][s, l] - e0["meanSATE"][s, l]) <= 1e-11 * abs(e0["meanSATE"][s, l]) + 1e-15
            assert abs(e1["varSATE"][s, l] - e0["varSATE"][s, l]) <= 1e-11 * abs(e0["varSATE"][s, l]) + 1e-14 * yS
        assert abs(e1["logpdf"][s] - e0["logpdf"][s]) <= 1e-11 * abs(e0["logpdf"][s])
    print(n, shape, bt, {k: f"{v:.2e}" for k, v in worst.items()})


def test_transforms_are_exact_where_they_claim_to_be():
    c = cases.make_case(24, "UX", False, S=2, seed=3)
    r = offscale.rescale_features(dict(c, baseline=np.array([0.1, 0.2])), (20, -20, 7), (-3, 11), 9)
    assert offscale.bits_equal(r["X"] * (1.0 / r["xyLS"][:, 0])[None, :], c["X"] * (1.0 / c["xyLS"][:, 0])[None, :])
    assert offscale.bits_equal(r["U"][:, :, 1] * (1.0 / r["uyLS"][:, 1])[None, :], c["U"][:, :, 1] * (1.0 / c["uyLS"][:, 1])[None, :])
    d0, d1 = c["T"] - c["doTs"][0], r["T"] - r["doTs"][0]
    assert offscale.bits_equal((d1 * d1) * (1.0 / (r["tyLS"][0] * r["tyLS"][0])), (d0 * d0) * (1.0 / (c["tyLS"][0] * c["tyLS"][0])))
    assert offscale.bits_equal(r["baseline"], np.array([0.1, 0.2]) * 512.0) and "baseline" not in c
    q = offscale.quantise(c, 12)
    s = offscale.fp32_shifted(q, 2.0 ** 13)
    assert offscale.bits_equal(s["X"] - 2.0 ** 13, q["X"]) and offscale.bits_equal(s["U"] - 2.0 ** 13, q["U"])
    assert offscale.bits_equal(s["T"] - s["doTs"][1], q["T"] - q["doTs"][1])
    assert np.max(np.abs(q["X"] - c["X"])) <= 2.0 ** -13
    o = offscale.rescale_outcome(c, -9)
    assert offscale.bits_equal(o["Y"] * 512.0, c["Y"]) and offscale.bits_equal(o["yNoise"] * 4.0 ** 9, c["yNoise"])
    # the comparison is on bits: -0.0 is not +0.0, a NaN equals itself
    assert not offscale.bits_equal(np.array([0.0]), np.array([-0.0])) and np.array([0.0]) == np.array([-0.0])
    assert offscale.bits_equal(np.array([np.nan]), np.array([np.nan]))
    assert not offscale.bits_equal(np.zeros(2), np.zeros((2, 1)))


def test_fp64_emulation_is_the_oracle():
    """The emulation at rt = float64 is the structured algebra: against the literal restatement at the golden tolerance."""
    c = cases.make_case(129, "UX", False, S=2, seed=5)
    e = cases.oracle_expected(c)
    ms, mi = offscale.emulate_kernel_mode(c, rt=np.float64)
    dm, di = offscale.drift(ms, mi, e["meanSATE"], e["meanITE"])
    assert dm <= 1e-9 and di <= 1e-9, (dm, di)


@pytest.fixture(scope="module")
def fp32_reference():
    """name -> (case, fp64 emulation of the unshifted case)."""
    return {k: (c, offscale.emulate_kernel_mode(c, rt=np.float64)) for k, c in offscale.fp32_base_cases().items()}


@pytest.mark.parametrize("name", ["main_L2", "main_L17", "X14", "binary"])
def test_centring_keeps_the_fp32_emulation_inside_its_budget(fp32_reference, name):
    c, ref = fp32_reference[name]
    for sh in offscale.FP32_SHIFTS:
        cs = offscale.fp32_shifted(c, sh)
        dm, di = offscale.drift(*offscale.emulate_kernel_mode(cs, centred=True), *ref)
        print(name, "shift", sh, "centred: meanSATE", f"{dm:.2e}", "MeanITE", f"{di:.2e}")
        assert dm < 5e-7 and di < 5e-7, (name, sh, dm, di)


@pytest.mark.parametrize("name", ["L2", "L9"])
def test_bridged_clusters_case_reaches_the_subnormal_exponents_inside_the_fp32_budget(name):
    c = offscale.bridged_cases()[name]
    x = c["X"][:, 0]
    a = (x[:, None] - x[None, :]) ** 2
    assert np.sum((a > 600) & (a < 900)) >= 1000 and np.sum((a > 708.4) & (a < 745.2)) >= 100 and a.max() > 3000
    dm, di = offscale.drift(*offscale.emulate_kernel_mode(c, centred=True), *offscale.emulate_kernel_mode(c, rt=np.float64))
    print("bridged", name, "centred: meanSATE", f"{dm:.2e}", "MeanITE", f"{di:.2e}")
    assert dm < 5e-7 and di < 5e-7, (dm, di)


def test_uncentred_fp32_emulation_breaks_the_budget_at_shift_100(fp32_reference):
    c, ref = fp32_reference["main_L2"]
    for sh in offscale.FP32_SHIFTS:
        dm, di = offscale.drift(*offscale.emulate_kernel_mode(offscale.fp32_shifted(c, sh), centred=False), *ref)
        print("shift", sh, "un-centred: meanSATE", f"{dm:.2e}", "MeanITE", f"{di:.2e}")
        if sh == 0.0:
            assert dm < 1e-6 and di < 1e-6, (dm, di)
        else:
            assert max(dm, di) > 1e-6, (sh, dm, di)


def test_longdouble_exp_is_math_exp_to_one_ulp_on_the_ladder():
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended long double"
    t = offscale.exp_ladder_t()
    a, ref = offscale.exp_reference(t)
    assert t[0] == 0.0 and a[0] == 0.0 and ref[0] == 1.0
    tiny = float(np.finfo(np.float64).tiny)
    assert np.any((ref > 0) & (ref < tiny)) and np.any(ref[a < 800] == 0.0) and np.any(a > 800) and np.isfinite(a).all()
    for aj, rj in zip(a, ref):
        try:
            m = math.exp(-aj)
        except OverflowError:      # not raised for underflow; kept for clarity
            m = 0.0
        assert abs(m - rj) <= offscale.ulp_distance_bound(np.array([rj]))[0], (aj, m, rj)
    # the ladder holds what it says: both sides of every breakpoint, the clamp, the subnormal edge
    ln2 = math.log(2.0)
    for bp in [ln2 / 2] + [ln2 / 64 * (2 * m + 1) for m in (0, 1, 2, 3, 15, 16, 31)]:
        assert np.any((a < bp) & (a > bp * (1 - 1e-15))) and np.any((a > bp) & (a < bp * (1 + 1e-15))), bp
    for v in (1.0, 37.4, 700.0, 708.39, 708.40, 744.4, 745.13, 745.14, 790.0, 800.0, 800.5, 1e4):
        assert np.min(np.abs(a - v)) <= 4e-16 * v, v
    assert 9.9e299 < a.max() < 1.01e300          # t = 1e150: the square is finite, far beyond the clamp
