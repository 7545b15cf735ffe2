"""The four level forms of the prediction path (ordinary, contrast, slope, outcome; csrc/level_form.h) against the bits recorded
BEFORE their table was folded into one header: every kernel that knows about levels (k_gram.hip, k_solve.hip, k_curve.hip,
k_vec.hip) now takes its per-form factors from LevelForm<FORM>, in the operation order the kernel had, so every output must be
equal BIT FOR BIT; a tolerance has no place here.  The older fixtures (predict_, tile_build_, pair_mfma_parent_hashes.json) hold
no slope, no outcome and no covW; this one does.  Unless noted the shape is n = 129 ("UX", S = 2): two tile columns with one live
row in the second.
  slope and outcome, plain:     L = 1, 2, 5 with MeanITE (the mean kernels' LCT = 1, LCT = 4 and MFMA rungs); L = 2 with seeded
                                draws, spp = 2 (dt_build, unit B); L = 40 at n = 200, sums only (the augmented row as a tile row
                                of its own)
  slope and outcome, weighted:  G = 3 with covW, L = 3 and L = 12 (37 right-hand sides: past the 32-row live_rows layout)
  ordinary and contrast, covW:  G = 3, L = 3; the contrast's middle level has a == b
  outcome at vector levels:     L = 2 with MeanITE and seeded draws
  ITEDistributions:             slope, outcome, outcome at a vector level
  shape "T" (F = 0):            slope and outcome, L = 2
tests/golden/level_form_parent_hashes.json holds the parent commit's hash and the SHA-256 of every output array the parent
returned on an MI355X, recorded twice in one process and the same both times."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level_form_parent_hashes.json")
OUT4 = ("meanSATE", "varSATE", "MeanITE", "draws")
CURVE = ("meanW", "varW", "covW", "MeanITE")
DIST = ("MeanITEs", "CovITEs")


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _named(names, arrays):
    return {k: _digest(a) for k, a in zip(names, arrays)}


def _obj(gp, seed, n=129, shape="UX"):
    return cases.gpslc_object(gp, cases.make_case(n, shape, False, S=2, seed=seed))


def _levels(L):
    return np.array([0.3]) if L == 1 else np.linspace(-0.6, 0.8, L)


def _form(form):
    return {form: True} if form in ("slope", "outcome") else {}


def _plain(gp, form, L):
    return _named(OUT4, gp.predict(_obj(gp, 800 + L), _levels(L), want_mean_ite=True, **_form(form)))


def _draws(gp, form):
    return _named(OUT4, gp.predict(_obj(gp, 810), _levels(2), want_mean_ite=True, spp=2, seed=5, want_draws=True, **_form(form)))


def _sums(gp, form):
    return _named(OUT4, gp.predict(_obj(gp, 811, n=200), _levels(40), **_form(form))[:2])


def _shape_t(gp, form):
    return _named(OUT4, gp.predict(_obj(gp, 812, shape="T"), _levels(2), want_mean_ite=True, **_form(form)))


def _weights(n, seed):
    rng = np.random.Generator(np.random.Philox(seed))
    return np.stack([np.full(n, 1.0 / n), rng.uniform(-1.0, 1.0, n) / n, (np.arange(n) % 3 == 0) / float(len(range(0, n, 3)))])


def _curve(gp, form, L):
    A = _levels(L)
    base = np.array([0.5, A[1], -0.5]) if form == "contrast" else None          # the middle level: a == b
    out, _ = gp.api._predict_curve(_obj(gp, 820 + L), A, baseline=base, weights=_weights(129, 8200 + L), want_mean_ite=True,
                                   **_form(form))
    return _named(CURVE, out[:4])


def _vector_levels(n, seed, L):
    return np.random.Generator(np.random.Philox(seed)).uniform(-1.0, 1.0, (L, n))


def _vec(gp):
    return _named(OUT4, gp.predict(_obj(gp, 830), _vector_levels(129, 8300, 2), want_mean_ite=True, spp=2, seed=6,
                                   want_draws=True, outcome=True))


def _ite_distributions(gp, form):
    g = _obj(gp, 840)
    if form == "outcome_vec":
        return _named(DIST, gp.ITEDistributions(g, _vector_levels(129, 8400, 1)[0], outcome=True))
    return _named(DIST, gp.ITEDistributions(g, 0.4, **_form(form)))


CASES = {}
for _f in ("slope", "outcome"):
    for _L in (1, 2, 5):
        CASES[f"{_f}_L{_L}"] = (_plain, _f, _L)
    CASES[f"{_f}_L2_draws"] = (_draws, _f)
    CASES[f"{_f}_L40_n200_sums"] = (_sums, _f)
    for _L in (3, 12):
        CASES[f"{_f}_G3_L{_L}_cov"] = (_curve, _f, _L)
    CASES[f"{_f}_T_L2"] = (_shape_t, _f)
for _f in ("ordinary", "contrast"):
    CASES[f"{_f}_G3_L3_cov"] = (_curve, _f, 3)
CASES["outcome_vec_L2"] = (_vec,)
for _f in ("slope", "outcome", "outcome_vec"):
    CASES[f"itedist_{_f}"] = (_ite_distributions, _f)


def compute(gp, case_id):
    fn, *args = CASES[case_id]
    return fn(gp, *args)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", list(CASES))
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    assert len(CASES) == 22
    assert sorted(recorded["hashes"]) == sorted(CASES)
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid, (fn, *_) in CASES.items():
        want = {_curve: CURVE, _ite_distributions: DIST, _sums: OUT4[:2], _plain: OUT4[:3], _shape_t: OUT4[:3]}.get(fn, OUT4)
        assert sorted(recorded["hashes"][cid]) == sorted(want), cid
