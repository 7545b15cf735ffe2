"""The device-pointer entry points — gpslc_predict_dev, gpslc_set_data_dev, gpslc_summarize_dev — with the caller's memory
under guard (tests/devmem.py): every input and every output of a call sits between two margins of one 128 x 128 tile of a
quiet-NaN pattern inside its own allocation.

The host-pointer entry points hand the kernels exactly-sized slices of the ctx's staging pool and copy out only the bytes
asked for: a store past the end of meanITE at the last ragged tile, or a read past the end of U or z, lands in the next slice
and nobody looks.  Under `_dev` the same accesses touch the caller's arrays.  Here

- gpslc_predict_dev must give the bits of gpslc_predict (same tuning, a second ctx), leave every output margin and every
  input bit untouched, and — one case per n — meet the oracle within the bounds of test_gpu_estimation.py /
  cases.draw_bounds;
- gpslc_set_data_dev must copy (the caller's arrays are overwritten afterwards);
- gpslc_summarize_dev must equal orc.summarize_estimates for the same logical n x m matrix stored contiguous, level-strided,
  row-major and with padded columns inside tensors whose other entries are plausible numbers, not zeros.

All shapes are small (n <= 300, S <= 8); nothing relies on, or tries to cause, a fault."""
import ctypes as C

import numpy as np
import pytest

import cases
import devmem
import gpslc_oracle as orc

pytestmark = pytest.mark.gpu

PN = 1e-3                 # predictionCovarianceNoise of every call here: cond(CovITE) stays small (cases.draw_bounds' tight bound)
SEED = 7
OUTS = ("meanSATE", "varSATE", "meanITE", "ite_draws")
LETTER = dict(m="meanSATE", v="varSATE", i="meanITE", d="ite_draws")
INPUTS = ("U", "uyLS", "xyLS", "tyLS", "yScale", "yNoise")


@pytest.fixture
def dev():
    yield devmem
    devmem.release()


def _levels(L):
    return np.array([0.25]) if L == 1 else np.linspace(-0.7, 0.9, L)


def _ctx(gp, c, fp32=False, tuning=None, schedule=None, ensemble=None, profile=False, set_data=True):
    nX = 0 if c["X"] is None else c["X"].shape[1]
    nU = 0 if c["U"] is None else c["U"].shape[1]
    ctx = gp.Context(c["n"], nX, nU, fp32_kernel=fp32, profile=profile)
    if set_data:
        ctx.set_data(c["X"], c["T"], c["Y"])
    if tuning:
        ctx.set_tuning(*tuning)
    if schedule:
        ctx.set_task_schedule(*schedule)
    if ensemble:
        ctx.set_ensemble(*ensemble)
    return ctx


def _sizes(n, S, L, spp):
    return dict(meanSATE=S * L, varSATE=S * L, meanITE=n * S * L, ite_draws=L * n * S * spp)


def _normals(c, L, spp, zmode):
    """the caller's z (n, spp, S, L), or None for the library's seeded stream"""
    if zmode != "caller" or spp == 0:
        return None
    return np.asfortranarray(np.random.default_rng(c["n"] + 10 * L + spp).standard_normal((c["n"], spp, c["S"], L)))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _predict_host(ctx, c, doTs, spp, z, want, S=None, L=None, null_doT=False):
    """gpslc_predict into host arrays pre-filled with the sentinel -> (status, {name: flat uint64})"""
    S = c["S"] if S is None else S
    L = len(doTs) if L is None else L
    size = _sizes(c["n"], c["S"], len(doTs), max(spp, 1))
    out = {k: (np.full(size[k], devmem.SENTINEL, dtype=np.uint64) if k in want else None) for k in OUTS}
    st = ctx.lib.gpslc_predict(ctx.h, S, *[_ptr(c[k]) for k in INPUTS], L, None if null_doT else _ptr(doTs), PN, spp, SEED,
                               _ptr(z), *[_ptr(out[k]) for k in OUTS])
    return st, out


class DevCall:
    """One gpslc_predict_dev call: every input in a guarded_up buffer, every requested output in a guarded one."""

    def __init__(self, dev, ctx, c, doTs, spp, z, want, S=None, L=None, null_doT=False):
        S = c["S"] if S is None else S
        L = len(doTs) if L is None else L
        size = _sizes(c["n"], c["S"], len(doTs), max(spp, 1))
        self.ins = {k: dev.guarded_up(c[k]) for k in INPUTS if c[k] is not None}
        self.ins["doT"] = dev.guarded_up(doTs)
        if z is not None:
            self.ins["z"] = dev.guarded_up(z)
        self.outs = {k: dev.guarded(size[k]) for k in OUTS if k in want}

        def p(bufs, k):
            return bufs[k].ptr if k in bufs else None

        self.status = ctx.lib.gpslc_predict_dev(ctx.h, S, *[p(self.ins, k) for k in INPUTS], L,
                                                None if null_doT else p(self.ins, "doT"), PN, spp, SEED, p(self.ins, "z"),
                                                *[p(self.outs, k) for k in OUTS])

    def inputs_untouched(self, dev):
        return [k for k, b in self.ins.items() if not dev.untouched(b)]

    def outputs_untouched(self, dev):
        return [k for k, b in self.outs.items() if not dev.untouched(b)]

    def broken_margins(self, dev):
        return [k for k, b in self.outs.items() if not dev.margins_intact(b)]


def _want(letters, spp):
    return tuple(LETTER[ch] for ch in letters if not (ch == "d" and spp == 0))


def _run_both(gp, dev, p):
    """the _dev call on one ctx and the host call on a second ctx with identical tuning"""
    c = cases.make_case(p["n"], p["shape"], False, S=p["S"], seed=p["n"] + p["S"])
    doTs = _levels(p["L"])
    z = _normals(c, p["L"], p["spp"], p["z"])
    want = _want(p["want"], p["spp"])
    kw = dict(fp32=p["fp32"], tuning=p["tuning"], schedule=p["schedule"], ensemble=p["ensemble"], profile=p["profile"])
    cd, chost = _ctx(gp, c, **kw), _ctx(gp, c, **kw)
    call = DevCall(dev, cd, c, doTs, p["spp"], z, want)
    st, ref = _predict_host(chost, c, doTs, p["spp"], z, want)
    return c, doTs, z, cd, chost, call, st, ref


def _assert_dev_equals_host(dev, c, cd, chost, call, st, ref):
    assert call.status == st == 0
    assert np.array_equal(cd.last_info(c["S"]), chost.last_info(c["S"]))
    for k, buf in call.outs.items():
        got = dev.interior_bits(buf)
        assert not np.any(got == devmem.SENTINEL), f"{k}: elements never written"
        assert not np.any(ref[k] == devmem.SENTINEL), f"{k}: host elements never written"
        assert np.array_equal(got, ref[k]), f"{k}: {int(np.sum(got != ref[k]))} of {got.size} words differ from gpslc_predict"
    assert call.broken_margins(dev) == []
    assert call.inputs_untouched(dev) == []


def P(id, n=129, shape="UX", S=2, L=3, spp=1, z="caller", want="mvid", fp32=False, tuning=None, schedule=None,
      ensemble=None, profile=False):
    return pytest.param(dict(n=n, shape=shape, S=S, L=L, spp=spp, z=z, want=want, fp32=fp32, tuning=tuning,
                             schedule=schedule, ensemble=ensemble, profile=profile), id=id)


TASKS = (0, -1, 1, 0)      # gpslc_set_task_schedule: the persistent task launch from one matrix on

PREDICT_CASES = (
    # one tile exactly or raggedly, two ragged tiles, three tiles; through the scatter (L = 3) and the direct draw store (L = 1)
    [P(f"n{n}", n=n) for n in (1, 127, 128, 129, 200, 300)]
    + [P(f"n{n}-L1-seeded", n=n, L=1, spp=3, z="seeded") for n in (1, 127, 128, 200)]
    # the four model shapes: NULL U / uyLS / xyLS
    + [P(f"shape{s}", shape=s) for s in ("U", "X", "T")]
    # L = 1 direct store, L = 3 scatter, L = 9 the MFMA MeanITE kernel; no draws, one, three; caller's z and Philox
    + [P(f"L{L}-spp0", L=L, spp=0) for L in (1, 3, 9)]
    + [P(f"L{L}-spp{spp}-{z}", L=L, spp=spp, z=z) for L in (1, 3, 9) for spp in (1, 3) for z in ("caller", "seeded")]
    + [P("n300-L1-spp3-seeded", n=300, L=1, spp=3, z="seeded"), P("n300-L9", n=300, L=9)]
    # chunks at s0 = 0, 2, 4 on alternating stream slots: the chunk offsets into the caller's arrays
    + [P("chunks-L1", S=5, L=1, tuning=(2, 0, 2)), P("chunks-L3", S=5, tuning=(2, 0, 2)),
       P("chunks-L3-seeded", S=5, spp=3, z="seeded", tuning=(2, 0, 2)), P("chunks-L9-spp0", S=5, L=9, spp=0, tuning=(2, 0, 2)),
       P("chunks-n300", n=300, S=5, tuning=(2, 0, 2))]
    # persistent task launch and per-column launches
    + [P("n300-tasks", n=300, S=5, schedule=TASKS, profile=True), P("n300-columns", n=300, S=5, profile=True)]
    # output subsets; the draws alone use the internal MeanITE scratch
    + [P(f"outputs-{w}", spp=3, want=w) for w in ("mvid", "m", "v", "i", "d")]
    + [P("fp32-L1", n=200, L=1, fp32=True), P("fp32-L3", n=200, fp32=True)]
    + [P("ensemble-L3", S=3, spp=3, z="seeded", ensemble=(2, 9)), P("ensemble-L1", S=3, L=1, spp=3, z="seeded", ensemble=(2, 9))]
)


@pytest.mark.parametrize("p", PREDICT_CASES)
def test_predict_dev_gives_the_bits_of_predict_and_stays_inside_its_arrays(gp, dev, p):
    c, doTs, z, cd, chost, call, st, ref = _run_both(gp, dev, p)
    _assert_dev_equals_host(dev, c, cd, chost, call, st, ref)
    if p["profile"]:           # the schedule asked for is the schedule that ran (profile class 4: potrf_tasks_kernel)
        launches = cd.profile_get(4)[0]
        assert (launches > 0) == (p["schedule"] is not None)


def test_predict_dev_bits_do_not_depend_on_the_schedule(gp, dev):
    """n = 300, S = 5: one persistent task launch against per-column launches, both through device pointers (the header of
    gpslc_set_task_schedule: every output is bit-identical either way)."""
    c = cases.make_case(300, "UX", False, S=5, seed=31)
    doTs, z = _levels(3), _normals(c, 3, 1, "caller")
    a = DevCall(dev, _ctx(gp, c, schedule=TASKS), c, doTs, 1, z, OUTS)
    b = DevCall(dev, _ctx(gp, c), c, doTs, 1, z, OUTS)
    assert a.status == b.status == 0
    for k in OUTS:
        assert np.array_equal(dev.interior_bits(a.outs[k]), dev.interior_bits(b.outs[k])), k
    assert a.broken_margins(dev) == [] and b.broken_margins(dev) == []


# worst error / bound of the _dev outputs against the oracle, per quantity (printed; pytest -s or -rP shows it)
WORST = dict(meanITE=0.0, meanSATE=0.0, varSATE=0.0, draws=0.0)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 200, 300])
def test_predict_dev_against_the_oracle(gp, dev, n):
    """Bit-identity with gpslc_predict compares two things that are both under test: here the downloaded _dev outputs against
    cases.oracle_expected and M + chol(C) z, within the bounds the host-path tests use — test_gpu_estimation.py's
    _check_against (SATE mean 1e-6 rel + 1e-12, variance 1e-6 rel + 1e-9 yScale, ITE mean 1e-6 max|ref| + 1e-12, and
    its `tight` 1e-9 guards) and cases.draw_bounds for the draws.  All outputs, L = 3, spp = 1, the caller's z."""
    S, L, spp = 2, 3, 1
    c = cases.make_case(n, "UX", False, S=S, seed=n + S)
    doTs = _levels(L)
    z = _normals(c, L, spp, "caller")
    call = DevCall(dev, _ctx(gp, c), c, doTs, spp, z, OUTS)
    assert call.status == 0
    assert call.broken_margins(dev) == [] and call.inputs_untouched(dev) == []
    ms = dev.interior(call.outs["meanSATE"]).reshape(S, L, order="F")
    vs = dev.interior(call.outs["varSATE"]).reshape(S, L, order="F")
    mi = dev.interior(call.outs["meanITE"]).reshape(n, S, L, order="F")
    dr = dev.interior(call.outs["ite_draws"]).reshape(L, n, S * spp, order="F")
    exp = cases.oracle_expected(dict(c, doTs=doTs), PN)
    worst = dict.fromkeys(WORST, 0.0)
    tight = 1e-9
    for s in range(S):
        for l in range(L):
            rm, rv, ref = exp["meanSATE"][s, l], exp["varSATE"][s, l], exp["meanITE"][:, s, l]
            em, ev_, ei = abs(ms[s, l] - rm), abs(vs[s, l] - rv), np.max(np.abs(mi[:, s, l] - ref))
            assert em <= 1e-6 * abs(rm) + 1e-12 and em <= tight * abs(rm) + 1e-13
            assert ev_ <= 1e-6 * abs(rv) + 1e-9 * c["yScale"][s] and ev_ <= tight * abs(rv) + 1e-12 * c["yScale"][s]
            assert ei <= 1e-6 * np.max(np.abs(ref)) + 1e-12 and ei <= tight * np.max(np.abs(ref)) + 1e-13
            worst["meanSATE"] = max(worst["meanSATE"], em / (tight * abs(rm) + 1e-13))
            worst["varSATE"] = max(worst["varSATE"], ev_ / (tight * abs(rv) + 1e-12 * c["yScale"][s]))
            worst["meanITE"] = max(worst["meanITE"], ei / (tight * np.max(np.abs(ref)) + 1e-13))
            Cv = exp["covITE"][s, l]                                   # carries + PN I
            lam = np.linalg.eigvalsh(Cv)
            draw = ref + np.linalg.cholesky(Cv) @ z[:, 0, s, l]
            err = np.linalg.norm(dr[l][:, s] - draw)
            bound, tb, cond = cases.draw_bounds(lam[0], lam[-1], np.linalg.norm(z[:, 0, s, l]), np.linalg.norm(draw))
            assert tb is not None, cond
            assert err <= bound and err <= tb, (s, l, err, tb)
            worst["draws"] = max(worst["draws"], err / tb)
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
    print(f"n = {n}: worst error / bound of the _dev outputs: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("so far over all n: " + ", ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


def test_predict_dev_with_no_samples_writes_nothing(gp, dev):
    """S = 0 returns 0 like gpslc_predict and leaves every output as it was, interior included."""
    c = cases.make_case(129, "UX", False, S=2, seed=3)
    doTs = _levels(3)
    z = _normals(c, 3, 1, "caller")
    cd, chost = _ctx(gp, c), _ctx(gp, c)
    call = DevCall(dev, cd, c, doTs, 1, z, OUTS, S=0)
    st, ref = _predict_host(chost, c, doTs, 1, z, OUTS, S=0)
    assert call.status == st == 0
    assert cd.last_info(0).size == 0 and chost.last_info(0).size == 0
    assert call.outputs_untouched(dev) == [] and call.inputs_untouched(dev) == []
    assert all(np.all(ref[k] == devmem.SENTINEL) for k in OUTS)


@pytest.mark.parametrize("what", ["null-doT", "L0", "draws-without-spp"])
def test_predict_dev_refusals_match_predict_and_touch_no_output(gp, dev, what):
    c = cases.make_case(129, "UX", False, S=2, seed=4)
    doTs = _levels(3)
    kw = dict(null_doT=True) if what == "null-doT" else dict(L=0) if what == "L0" else {}
    spp = 0 if what == "draws-without-spp" else 1
    z = _normals(c, 3, 1, "caller")
    cd, chost = _ctx(gp, c), _ctx(gp, c)
    call = DevCall(dev, cd, c, doTs, spp, z, OUTS, **kw)
    st, ref = _predict_host(chost, c, doTs, spp, z, OUTS, **kw)
    assert call.status == st and st < 0 and st > -100, (call.status, st)     # "argument #k is invalid", the same k
    assert call.outputs_untouched(dev) == [] and call.inputs_untouched(dev) == []
    assert all(np.all(ref[k] == devmem.SENTINEL) for k in OUTS)


# ---- gpslc_set_data_dev ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,binary", [("UX", False), ("U", False), ("X", True)])
def test_set_data_dev_copies_the_callers_arrays(gp, dev, shape, binary):
    """A ctx built from guarded device copies of X, T, Y (X NULL when nX = 0) predicts the bits of one built with
    gpslc_set_data, reads nothing beyond the arrays, and keeps predicting them after the caller has overwritten its buffers:
    the library copies (include/gpslc_hip.h: the caller may free or reuse its arrays after the call)."""
    c = cases.make_case(129, shape, binary, S=3, seed=9)
    doTs = np.array([0.0, 1.0]) if binary else _levels(2)
    want = OUTS
    st, ref = _predict_host(_ctx(gp, c), c, doTs, 2, None, want)
    assert st == 0
    bufs = {k: dev.guarded_up(c[k]) for k in ("X", "T", "Y") if c[k] is not None}
    ctx = _ctx(gp, c, set_data=False)
    ctx.check(ctx.lib.gpslc_set_data_dev(ctx.h, bufs["X"].ptr if "X" in bufs else None, bufs["T"].ptr, bufs["Y"].ptr))
    assert [k for k, b in bufs.items() if not dev.untouched(b)] == []
    st, got = _predict_host(ctx, c, doTs, 2, None, want)
    assert st == 0
    for k in want:
        assert np.array_equal(got[k], ref[k]), k
    for b in bufs.values():
        dev.overwrite(b)                        # the caller reuses its arrays
    st, again = _predict_host(ctx, c, doTs, 2, None, want)
    assert st == 0
    for k in want:
        assert np.array_equal(again[k], ref[k]), k


# ---- gpslc_summarize_dev ---------------------------------------------------------------------------------------------------

LAYOUTS = ("contiguous", "level", "rowmajor", "padded")
LVL = 3


def _sample_matrix(rng, n, m):
    """scaled, shifted normals; rows with heavy ties, all negative, constant, and holding both zeros (where n has the rows)"""
    x = rng.standard_normal((n, m)) * rng.uniform(0.1, 10, (n, 1)) + rng.uniform(-3, 3, (n, 1))
    if n > 1:
        x[1] = np.round(x[1])                      # many duplicates around the quantiles
    if n > 2:
        x[2] = -np.abs(x[2]) - 0.5
    if n > 3:
        x[3, :] = 2.5                              # a constant row
    if n > 4:
        x[4, ::3] = 0.0
        x[4, 1::3] = -0.0
    return x


def _store(rng, layout, n, m):
    """-> (the tensor as it lies in memory (flat), [(x, offset, row_stride, col_stride)]): logical n x m matrices inside it"""
    if layout == "level":                          # L x n x M, level fastest: one matrix per level
        xs = [_sample_matrix(rng, n, m) for _ in range(LVL)]
        t = np.stack(xs)                           # (L, n, m)
        return t.reshape(-1, order="F"), [(xs[l], l, LVL, LVL * n) for l in range(LVL)]
    x = _sample_matrix(rng, n, m)
    if layout == "contiguous":
        return x.reshape(-1, order="F"), [(x, 0, 1, n)]
    if layout == "rowmajor":
        return x.reshape(-1, order="C"), [(x, 0, m, 1)]
    t = np.vstack([x, rng.standard_normal((5, m)) * 4.0])          # padded columns: n + 5 rows
    return t.reshape(-1, order="F"), [(x, 0, 1, n + 5)]


def _summarize_and_check(dev, ctx, tensor_buf, x, offset, rs, cs, cis=(0.9, 0.5)):
    n, m = x.shape
    for ci in cis:
        o = [dev.guarded(n) for _ in range(3)]
        st = ctx.lib.gpslc_summarize_dev(ctx.h, tensor_buf.at(offset), n, m, rs, cs, ci, o[0].ptr, o[1].ptr, o[2].ptr)
        assert st == 0, (st, ctx.lib.gpslc_last_error(ctx.h))
        mean, lo, hi = orc.summarize_estimates(x, ci)
        got = [dev.interior(b) for b in o]
        assert all(dev.margins_intact(b) for b in o)
        assert np.array_equal(got[1], lo) and np.array_equal(got[2], hi), (n, m, offset, rs, cs, ci)
        if m <= 16384:                             # the bounds of test_summarize_estimates_on_device
            assert np.allclose(got[0], mean, rtol=1e-14, atol=1e-16), np.max(np.abs(got[0] - mean) / np.abs(mean))
        else:
            assert np.allclose(got[0], mean, rtol=1e-13, atol=1e-15), np.max(np.abs(got[0] - mean) / np.abs(mean))
    assert dev.untouched(tensor_buf)


def _summarize_case(gp, dev, layout, n, m):
    rng = np.random.default_rng(1000 * n + m)
    flat, views = _store(rng, layout, n, m)
    ctx = gp.Context(1, 0, 0)
    buf = dev.guarded_up(flat)
    for x, offset, rs, cs in views:
        _summarize_and_check(dev, ctx, buf, x, offset, rs, cs)


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 1000, 16384, 16385, 20000])
def test_summarize_dev_level_strided_at_every_row_length(gp, dev, m):
    """n = 17 (a dead-row group in the select kernel), every level of an L x n x M tensor summarised in place: the LDS sort with
    mpad below, at and above one 256-thread pass and at the full image (m <= 16384), the radix select beyond."""
    _summarize_case(gp, dev, "level", 17, m)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", [1000, 16385])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_summarize_dev_layouts(gp, dev, n, m, layout):
    """The same logical matrix contiguous (1, n), level-strided (L, L n), row-major (m, 1) and with padded columns (1, n + 5),
    for the sort (m = 1000) and the select kernel (m = 16385: 16 rows per workgroup, n = 17 and 33 leave dead rows)."""
    _summarize_case(gp, dev, layout, n, m)


def test_summarize_dev_in_place_on_the_draws_of_predict_dev(gp, dev):
    """End to end as include/gpslc_hip.h describes it: gpslc_predict_dev leaves its L x n x (S spp) draw tensor on the device,
    every level is summarised from it with samples = draws + l, row_stride = L, col_stride = L n; the tensor is unchanged."""
    n, S, L, spp = 200, 4, 3, 50
    c = cases.make_case(n, "UX", False, S=S, seed=21)
    doTs = _levels(L)
    z = np.asfortranarray(np.random.default_rng(5).standard_normal((n, spp, S, L)))
    ctx = _ctx(gp, c)
    call = DevCall(dev, ctx, c, doTs, spp, z, ("ite_draws",))
    assert call.status == 0 and call.broken_margins(dev) == []
    buf = call.outs["ite_draws"]
    buf.bits = dev.interior_bits(buf)              # what predict_dev left: must survive the summaries
    draws = buf.bits.view(np.float64).reshape(L, n, S * spp, order="F")
    assert np.all(np.isfinite(draws))
    for l in range(L):
        _summarize_and_check(dev, ctx, buf, np.ascontiguousarray(draws[l]), l, L, L * n, cis=(0.9,))


def test_summarize_dev_argument_statuses(gp, dev):
    """minus the number of the offending argument; a refused call writes nothing.  The strides are refused when below 1 (a
    zero or negative stride is never a layout of an n x m matrix): samples points at the middle of a guarded buffer and
    n |row_stride| + m |col_stride| stays far below PAD."""
    n, m = 4, 8
    buf = dev.guarded_up(np.random.default_rng(2).standard_normal(4096))
    mid = buf.at(2048)
    o = [dev.guarded(n) for _ in range(3)]
    ctx = gp.Context(1, 0, 0)
    f = ctx.lib.gpslc_summarize_dev
    ptrs = [b.ptr for b in o]
    assert f(ctx.h, None, n, m, 1, n, 0.9, *ptrs) == -2
    assert f(ctx.h, mid, 0, m, 1, n, 0.9, *ptrs) == -3
    assert f(ctx.h, mid, -1, m, 1, n, 0.9, *ptrs) == -3
    assert f(ctx.h, mid, n, 0, 1, n, 0.9, *ptrs) == -4
    for rs in (0, -1):
        assert f(ctx.h, mid, n, m, rs, n, 0.9, *ptrs) == -5
    for cs in (0, -n):
        assert f(ctx.h, mid, n, m, 1, cs, 0.9, *ptrs) == -6
    for ci in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert f(ctx.h, mid, n, m, 1, n, ci, *ptrs) == -7
    for k in range(3):
        assert f(ctx.h, mid, n, m, 1, n, 0.9, *[None if j == k else p for j, p in enumerate(ptrs)]) == -8
    assert all(dev.untouched(b) for b in o) and dev.untouched(buf)
    assert f(ctx.h, mid, n, m, 1, n, 0.9, *ptrs) == 0          # and the same arguments, valid, go through
    assert all(dev.margins_intact(b) for b in o) and dev.untouched(buf)
    x = buf.bits.view(np.float64)[2048:2048 + n * m].reshape(n, m, order="F")
    mean, lo, hi = orc.summarize_estimates(x, 0.9)
    assert np.array_equal(dev.interior(o[1]), lo) and np.array_equal(dev.interior(o[2]), hi)
