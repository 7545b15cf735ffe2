"""The two MFMA pair kernels against results recorded BEFORE they were folded onto one pair-product body (csrc/pair_mfma.h):
ite_mean_mfma_kernel (k_solve.hip: MeanITE of L > 4 levels, plain and contrast) and wsum_mfma_kernel (k_wsum.hip: BW = B W and
KW = K W of weighted effects, with K, without K for contrasts, and the binary-treatment shortcut).  The fold keeps every
floating-point operation and its order, and giving wsum the mean kernel's FREG ladder only changes how many zero features pad
a pair (fma(0 - 0, 0 - 0, lux) with lux >= +0 returns lux), so every output must be equal BIT FOR BIT; a tolerance has no
place here.
tests/golden/pair_mfma_parent_hashes.json holds the parent commit's hash and the SHA-256 of meanSATE, varSATE and MeanITE that
the parent returned on an MI355X for the seeded cases below (S = 2, so the batch index is nonzero), the smallest shapes at which
each branch of the shared body can go wrong:
  - feature sweep at n = 200 (two row tiles, the second ragged with its last 64-column chunk wholly beyond n) and L = 17 (two
    live 16-column sub-tiles, the second with one live column): F = 0, 3, 4, 5, 8, 10 (recorded with wsum's FREG = 12), 12,
    14 (features from LDS) and 32 (the LDS opt-in limit), each as plain levels with one level equal to a T[i], contrasts with
    one pair a == b, weights G = 3, weights with a baseline (wsum without K) and a binary treatment with weights (BIN);
  - column passes at F = 5: L = 5, 16, 64, 70 (a second pass of 6 live columns) plain and contrast, G = 1, 16, 70 at L = 1
    with and without a baseline;
  - sizes at F = 5, L = 17: n = 128 (one full tile), 129 (one live row and column in the second tile), 257 (three tiles), plain
    and weighted.
Every output was recorded twice on the parent in one process and was the same both times.
The work replaced: src/estimation.jl:36-163."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_mfma_parent_hashes.json")
OUT3 = ("meanSATE", "varSATE", "MeanITE")
FEATURES = (("T", 0, 0), ("UX", 1, 2), ("UX", 1, 3), ("UX", 2, 3), ("UX", 2, 6), ("UX", 2, 8), ("UX", 4, 8), ("UX", 5, 9),
            ("UX", 8, 24))                         # (shape, nU, nX): F = 0, 3, 4, 5, 8, 10, 12, 14, 32
FORMS = ("plain", "contrast", "weighted", "weighted_base", "binary_weighted")
F5 = ("UX", 2, 3)


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _weights(n, G, seed):
    """G weight rows: the SATE weights, then signed Philox weights, with a group mask (as its average) every third row."""
    rng = np.random.Generator(np.random.Philox(seed))
    W = rng.uniform(-1.0, 1.0, (G, n)) / n
    W[0] = 1.0 / n
    for g in range(2, G, 3):
        W[g] = (np.arange(n) % 3 == g % 3) / float(len(range(g % 3, n, 3)))
    return W


def _run(gp, n, feat, form, L, G, seed):
    shape, nU, nX = feat
    c = cases.make_case(n, shape, form == "binary_weighted", S=2, nU=max(nU, 1), nX=max(nX, 1), seed=seed)
    g = cases.gpslc_object(gp, c)
    levels = np.linspace(-0.6, 0.8, L)
    base = W = None
    if form == "plain":
        levels[L // 2] = c["T"][n // 3]            # MeanITE[n // 3, :, L // 2] is the exact-zero row rule's
    if form in ("contrast", "weighted_base"):
        base = np.linspace(0.5, -0.5, L)
        if L > 1:
            base[L - 1] = levels[L - 1]            # one pair a == b
    if form in ("weighted", "weighted_base", "binary_weighted"):
        W = _weights(n, G, 7000 + seed)
    out = gp.predict(g, levels, baseline=base, weights=W, want_mean_ite=True)
    g.ctx().close()
    return {k: _digest(a) for k, a in zip(OUT3, out)}


CASES = {}
for _i, _f in enumerate(FEATURES):
    for _j, _form in enumerate(FORMS):
        CASES[f"F{_f[1] + _f[2]}_{_form}"] = (200, _f, _form, 17, 3, 100 + 10 * _i + _j)
for _i, _L in enumerate((5, 16, 64, 70)):
    CASES[f"L{_L}_plain"] = (200, F5, "plain", _L, 0, 300 + 2 * _i)
    CASES[f"L{_L}_contrast"] = (200, F5, "contrast", _L, 0, 301 + 2 * _i)
for _i, _G in enumerate((1, 16, 70)):
    CASES[f"G{_G}_weighted"] = (200, F5, "weighted", 1, _G, 320 + 2 * _i)
    CASES[f"G{_G}_weighted_base"] = (200, F5, "weighted_base", 1, _G, 321 + 2 * _i)
for _i, _n in enumerate((128, 129, 257)):
    CASES[f"n{_n}_plain"] = (_n, F5, "plain", 17, 0, 340 + 2 * _i)
    CASES[f"n{_n}_weighted"] = (_n, F5, "weighted", 17, 3, 341 + 2 * _i)


def case_ids():
    return list(CASES)


def compute(gp, case_id):
    return _run(gp, *CASES[case_id])


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, with every output, and the parent's second run gave the first one's bits."""
    assert len(case_ids()) == 65
    assert sorted(recorded["hashes"]) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in case_ids():
        assert sorted(recorded["hashes"][cid]) == sorted(OUT3), cid
