"""The two pair kernels of unit A — the Gram build (gram_kernel, k_gram.hip) and the MeanITE pass (k_solve.hip) — against the
results the parent commit returned, at sizes the older fixtures do not reach.  Those stop at n = 200, where every Gram tile is
padded or diagonal and the MeanITE pass sees two column tiles; the cases here have interior tiles, full diagonal tiles, a tile row
with one live row, and three or four column tiles per row block.

The MeanITE pass now takes the column's features and level values through scalar loads from a per-sample operand array
(ite_mean_sop_kernel) instead of staging them in LDS per workgroup.  The change keeps every floating-point operation of a pair,
its operands and its order, and the order in which a row's pairs are added (columns 0..63 and 64..127 of each column tile in two
chains, ascending over the tiles, then one addition), so every output must be equal BIT FOR BIT; a tolerance has no place here.

tests/golden/pair_scalar_parent_hashes.json holds the parent commit's hash and the SHA-256 of meanSATE, varSATE and MeanITE of
predict(want_mean_ite=True) as the parent returned them on an MI355X for the seeded cases below; S = 2, so the batch index is
nonzero.  Every case was recorded twice in one process and was the same both times.

  n384_F5_L1            three full tiles per side: the interior tiles (1,0), (2,0), (2,1) take the Gram kernel's FAST path, the
                        diagonal tiles are full
  n385_F10_L1           the benchmark's feature width; a fourth tile row with one live row: rectangular edge tiles and identity
                        padding beside FAST tiles
  n300_F7_L3            the runtime-F Gram path, and the LCT = 4 rung of the MeanITE pass with a partly filled level block
  n257_F4_binary_L1     binary treatments (BIN); one live row in the third tile row
  n200_F32_L2           MAXF: the MeanITE rung that keeps its LDS staging (32 features do not fit the scalar registers)
  n384_F5_contrast_L2   a paired level form (a != b) through the level vectors R
  n384_F5_sate_only     want_mean_ite=False: the SATE sums alone
"""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_scalar_parent_hashes.json")
OUTPUTS = ("meanSATE", "varSATE", "MeanITE")
#            n, (nU, nX), binary T, L, contrast, want_mean_ite, seed
CASES = {
    "n384_F5_L1": (384, (2, 3), False, 1, False, True, 600),
    "n385_F10_L1": (385, (2, 8), False, 1, False, True, 601),
    "n300_F7_L3": (300, (2, 5), False, 3, False, True, 602),
    "n257_F4_binary_L1": (257, (1, 3), True, 1, False, True, 603),
    "n200_F32_L2": (200, (8, 24), False, 2, False, True, 604),
    "n384_F5_contrast_L2": (384, (2, 3), False, 2, True, True, 605),
    "n384_F5_sate_only": (384, (2, 3), False, 1, False, False, 606),
}


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def case_ids():
    return list(CASES)


def outputs_of(case_id):
    return OUTPUTS if CASES[case_id][5] else OUTPUTS[:2]


def compute(gp, case_id):
    n, (nU, nX), binary, L, contrast, want_mean, seed = CASES[case_id]
    c = cases.make_case(n, "UX", binary, S=2, nU=nU, nX=nX, seed=seed)
    g = cases.gpslc_object(gp, c)
    if binary:
        levels = np.array([1.0])
    else:
        levels = np.linspace(-0.6, 0.8, L) if L > 1 else np.array([0.4])
    base = np.linspace(0.5, -0.5, L) if contrast else None
    out = gp.predict(g, levels, baseline=base, want_mean_ite=want_mean)
    g.ctx().close()
    return {k: _digest(a) for k, a in zip(outputs_of(case_id), out)}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    got = compute(gp, case_id)
    print(case_id, got)
    assert got == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, with every output, and the parent's second run gave the first one's bits."""
    assert len(case_ids()) == 7
    assert sorted(recorded["hashes"]) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in case_ids():
        assert sorted(recorded["hashes"][cid]) == sorted(outputs_of(cid)), cid
