"""The outcome-model entry points that ride on the tiled factor (gpslc_y_loo, gpslc_y_lgo, gpslc_y_logpdf_grad, gpslc_predict_new)
against results recorded BEFORE their host side was folded together: one body for the calls at the C boundary, the features'
members of PredictIO grouped, one sub-batch loop for the pair workspaces of unit B and of the new individuals, one plan for the
four Context methods (api_score.hip, predict.hip, api.py).  None of that touches a kernel or reorders a floating-point operation, so every output
must be equal BIT FOR BIT; a tolerance has no place here.  tests/golden/outcome_parent_hashes.json holds the parent commit's hash
and the SHA-256 of every output the parent returned on an MI355X for the seeded cases below, at the smallest sizes that reach
each path: tiles are 128 wide, so n = 200 is two tiles and n = 300 three with a ragged last one.

For each of y_loo, y_lgo and y_logpdf_grad (every output and logpdf): both sizes with U and X; n = 200 without U, without X, with
neither, and with a binary treatment; S = 5 in chunks of two on two streams (equal to the default tuning's bits); both
factorisation schedules (equal bits); both overrides; one output asked alone (equal to that output of the full call); a sample
whose factorisation breaks down (NaN pattern, status and last_info); an fp32-kernel context (the gradient refuses it: its
status).  y_lgo also with groups of 128 and 127 beside singletons and pairs under shuffled label ids, and with every individual
a group of its own.  predict_new at n = 200: the three forms, one new individual and 130 (two row tiles), each combination of
outputs, and 130 (sample, level) pairs for sub-batches of 128; unit B's draws with 130 pairs likewise (no other fixture has a
draws call with more pairs than one sub-batch).  Every output was repeatable on the parent (two runs of `compute` in one process
gave the same hashes: the fixture's "second_run"), so none is left out."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases
import new_individuals_restatement as nr

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outcome_parent_hashes.json")
CALLS = ("loo", "lgo", "grad")
LOO_OUT = ("mean", "var", "lpd", "logpdf")
ALONE = {"loo": "var", "lgo": "lpd", "grad": "dU"}          # the output asked alone, one per function
TUNED, DEFAULT = "n300_S5_chunks_of_2_on_2_streams", "n300_S5_default_tuning"
SCHEDULES = {"n300_task_launch": (2, 32, 1, 0), "n300_panel_launches": (2, 0, 1, 0)}
NEW_WANTS = {"mean": ("mean",), "mean_var": ("mean", "var"), "all": ("mean", "var", "cov")}


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _labels(n, how):
    if how == "mod7":
        return 7, (np.arange(n) % 7).astype(np.int32)
    if how == "singletons":
        return n, np.arange(n, dtype=np.int32)
    # n = 300: one group of 128, one of 127, the other 45 individuals as 15 pairs and 15 singletons; rows and label ids shuffled
    assert how == "big_groups" and n == 300
    sizes = [128, 127] + [2] * 15 + [1] * 15
    rng = _rng(8300)
    lab = np.empty(n, dtype=np.int32)
    lab[rng.permutation(n)] = np.repeat(rng.permutation(len(sizes)), sizes)
    return len(sizes), lab


def _call(fn, g, Xo=None, Yo=None, labels="mod7", want=None):
    """one Context call with every output (or `want`): {"status", outputs..., "last_info"}"""
    ctx, S = g.ctx(), g.getNumPosteriorSamples()
    args = (S, g.U, Xo, Yo, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    kw = {} if want is None else {"want": want}
    if fn == "grad":
        st, out = ctx.y_logpdf_grad(*args, **kw)
        out = {k: v for k, v in out.items() if v is not None}
    else:
        st, *arrays = ctx.y_loo(*args, **kw) if fn == "loo" else ctx.y_lgo(*args, *_labels(g.getN(), labels), **kw)
        out = {k: v for k, v in zip(LOO_OUT, arrays) if v is not None}
    res = {k: _digest(v) for k, v in out.items()}
    res["status"] = int(st)
    if st >= 0:
        res["last_info"] = _digest(ctx.last_info(S))
    return res


def _plain(gp, fn, n, shape, binary_t, S=3, tuning=None, schedule=None, fp32=False, labels="mod7", want=None):
    c = cases.make_case(n, shape, binary_t, S=S, seed=83)
    g = cases.gpslc_object(gp, c, **({"fp32_kernel": True} if fp32 else {}))
    if tuning:
        g.ctx().set_tuning(**tuning)
    if schedule:
        g.ctx().set_task_schedule(*schedule)
    return _call(fn, g, labels=labels, want=want)


def _overrides(gp, fn):
    c = cases.make_case(200, "UX", False, S=3, seed=83)
    rng = _rng(8200)
    return _call(fn, cases.gpslc_object(gp, c), Xo=np.asfortranarray(rng.standard_normal(c["X"].shape)), Yo=rng.standard_normal(200))


def _broken_case():
    """every suite's test_breakdown_gives_nan_for_that_sample_only: yNoise = 0 and a duplicated individual in a model without U
    and X, so that pivot 2 of sample 0 is exactly 0"""
    c = dict(cases.make_case(200, "T", False, S=2, seed=84))
    c["T"] = c["T"].copy()
    c["T"][1] = c["T"][0]
    c["yScale"] = np.array([1.0, c["yScale"][1]])
    c["yNoise"] = np.array([0.0, c["yNoise"][1]])
    return c


def _breakdown(gp, fn):
    return _call(fn, cases.gpslc_object(gp, _broken_case()))


def _new(gp, form, m, L, want, broken=False):
    c = _broken_case() if broken else cases.make_case(200, "UX", False, S=2, seed=85)
    g = cases.gpslc_object(gp, c)
    Xn, Un = nr.new_individuals(c, m, seed=m + L)
    lv = nr.pairs(form, L)
    doT = np.array([a for a, _ in lv])
    base = np.array([b for _, b in lv]) if form == "contrast" else None
    st, *arrays = g.ctx().predict_new(2, g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, Xn, Un, form, doT, base, nr.PN,
                                      want=NEW_WANTS[want])
    res = {k: _digest(v) for k, v in zip(("mean", "var", "cov"), arrays) if v is not None}
    res["status"] = int(st)
    res["last_info"] = _digest(g.ctx().last_info(2))
    return res


def _draws(gp):
    """unit B through the shared sub-batch loop: S = 2, L = 65 are 130 pairs for sub-batches of 128"""
    g = cases.gpslc_object(gp, cases.make_case(200, "UX", False, S=2, seed=86))
    out = gp.predict(g, np.linspace(-0.6, 0.8, 65), want_mean_ite=True, spp=2, seed=8600, want_draws=True)
    return {k: _digest(v) for k, v in zip(("meanSATE", "varSATE", "meanITE", "draws"), out)}


CASES = {}
for _fn in CALLS:
    for _n in (200, 300):
        CASES[f"{_fn}_n{_n}_UX"] = (_plain, _fn, _n, "UX", False)
    for _shape in ("U", "X", "T"):
        CASES[f"{_fn}_n200_{_shape}"] = (_plain, _fn, 200, _shape, False)
    CASES[f"{_fn}_n200_UX_binary"] = (_plain, _fn, 200, "UX", True)
    CASES[f"{_fn}_{TUNED}"] = (_plain, _fn, 300, "UX", False, 5, dict(max_batch=2, n_streams=2))
    CASES[f"{_fn}_{DEFAULT}"] = (_plain, _fn, 300, "UX", False, 5)
    for _name, _sched in SCHEDULES.items():
        CASES[f"{_fn}_{_name}"] = (_plain, _fn, 300, "UX", False, 3, None, _sched)
    CASES[f"{_fn}_n200_overrides"] = (_overrides, _fn)
    CASES[f"{_fn}_n200_{ALONE[_fn]}_alone"] = (_plain, _fn, 200, "UX", False, 3, None, None, False, "mod7", (ALONE[_fn],))
    CASES[f"{_fn}_breakdown"] = (_breakdown, _fn)
    CASES[f"{_fn}_n200_fp32"] = (_plain, _fn, 200, "UX", False, 3, None, None, True)
CASES["lgo_n300_big_groups"] = (_plain, "lgo", 300, "UX", False, 3, None, None, False, "big_groups")
CASES["lgo_n200_singletons"] = (_plain, "lgo", 200, "UX", False, 3, None, None, False, "singletons")
for _form in nr.FORMS:
    for _m in (1, 130):
        for _want in NEW_WANTS:
            CASES[f"new_{_form}_m{_m}_{_want}"] = (_new, _form, _m, 3, _want)
    CASES[f"new_{_form}_m5_L65_all"] = (_new, _form, 5, 65, "all")
CASES["new_outcome_m130_L65_mean_var"] = (_new, "outcome", 130, 65, "mean_var")
CASES["new_outcome_breakdown"] = (_new, "outcome", 3, 2, "all", True)
CASES["draws_n200_L65_spp2"] = (_draws,)


def case_ids():
    return list(CASES)


def compute(gp, case_id):
    fn, *args = CASES[case_id]
    return fn(gp, *args)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_outcome_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_fixture_holds_exactly_the_cases_and_the_parent_repeated_itself(recorded):
    """The fixture itself: every case is there, the parent's second run gave the first one's hashes, chunks on alternating
    streams and both schedules gave the bits of the default call, and an output asked alone those of the full call."""
    h = recorded["hashes"]
    assert sorted(h) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert h == recorded["second_run"]
    for fn in CALLS:
        assert h[f"{fn}_{TUNED}"] == h[f"{fn}_{DEFAULT}"], fn
        a, b = (h[f"{fn}_{name}"] for name in SCHEDULES)
        assert a == b, fn
        alone = h[f"{fn}_n200_{ALONE[fn]}_alone"]
        assert alone[ALONE[fn]] == h[f"{fn}_n200_UX"][ALONE[fn]], fn
        assert h[f"{fn}_breakdown"]["status"] == 2, fn
    assert h["grad_n200_fp32"]["status"] < 0 and h["loo_n200_fp32"]["status"] == h["lgo_n200_fp32"]["status"] == 0
