"""The predictive draws (gpslc_predict's unit C: out[:, d] = MeanITE + L_c z[:, d]) against results recorded BEFORE every draw
count was served by passes of the streaming draw kernel (csrc/k_draws.hip) and the Philox normal got one definition
(csrc/philox.h).  On the parent, units of more than 128 draws ran an LDS-staged MFMA kernel with a generator kernel of its own;
both kernels issue the same 16x16x4 f64 MFMAs with the same operands in the same ascending order of 4-column groups, every
draw has an accumulator of its own, and the Philox expressions are kept as they stood, so every draw must be equal BIT FOR
BIT; a tolerance has no place here.
tests/golden/draws_parent_hashes.json holds the parent commit's hash and the SHA-256 of the draw tensor the parent returned on
an MI355X for the cases below (S = 2, L = 1, predictionCovarianceNoise = 1e-3 unless the case says otherwise):
  - n = 129 (odd, one live row in tile 2), 256 (even, two full tiles: the pair branch of the staging) and 383 (nt = 3: the
    middle tile row has no partner), each with spp = 1, 16, 17, 33, 65 (every block count of the kernel), 128 (one pass exactly
    full), 129, 130 (one and two draws into a second pass), 256 (two full passes), 257 (two full passes and one draw) and 300
    (a ragged third pass), seeded and with a caller's z;
  - at n = 383: L = 3 with spp = 10 and 130 (staging strides and the level-sweep scatter), spp = 130 seeded under
    gpslc_set_ensemble(5, 140), and spp = 130, L = 3 under gpslc_set_tuning(3, 0, 2) (later sub-batches).
Every output was recorded twice on the parent in one process and was the same both times.
The work replaced: src/estimation.jl:95-109, src/prediction.jl:30-33."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draws_parent_hashes.json")
PN = 1e-3
S = 2
NS = (129, 256, 383)
SPPS = (1, 16, 17, 33, 65, 128, 129, 130, 256, 257, 300)
FORMS = ("seeded", "z")


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _run(gp, n, spp, L, form, ensemble, tuning):
    c = cases.make_case(n, "UX", False, S=S, seed=1000 + n)
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=PN))
    if tuning:
        g.ctx().set_tuning(*tuning)
    if ensemble:
        g.ctx().set_ensemble(*ensemble)
    doTs = np.linspace(-0.4, 0.7, L)
    seed = 5000 + 7 * n + spp + L
    z = None
    if form == "z":
        z = np.random.Generator(np.random.Philox(seed)).standard_normal((n, spp, S, L))
    dr = gp.predict(g, doTs, spp=spp, z=z, seed=0 if form == "z" else seed, want_draws=True)[3]
    g.ctx().close()
    assert dr.shape == (L, n, S * spp)
    return {"draws": _digest(dr)}


CASES = {}
for _n in NS:
    for _spp in SPPS:
        for _form in FORMS:
            CASES[f"n{_n}_spp{_spp}_{_form}"] = (_n, _spp, 1, _form, None, None)
for _spp in (10, 130):
    for _form in FORMS:
        CASES[f"n383_spp{_spp}_L3_{_form}"] = (383, _spp, 3, _form, None, None)
CASES["n383_spp130_seeded_ensemble"] = (383, 130, 1, "seeded", (5, 140), None)
for _form in FORMS:
    CASES[f"n383_spp130_L3_{_form}_tuning"] = (383, 130, 3, _form, None, (3, 0, 2))


def case_ids():
    return list(CASES)


def compute(gp, case_id):
    return _run(gp, *CASES[case_id])


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_draws_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, and the parent's second run gave the first one's bits."""
    assert len(case_ids()) == 73
    assert sorted(recorded["hashes"]) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in case_ids():
        assert sorted(recorded["hashes"][cid]) == ["draws"], cid
