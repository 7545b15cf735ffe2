"""likelihoodDistribution's W1 = K L^-T and W2 = Ks' L^-T against the bits recorded BEFORE the solve went through w_solve
(predict.hip): one strip-kernel launch per tile column, column update and panel product in one work item, instead of a column
update by the trailing kernel followed by that kernel's stand-alone panel product.  Per output element both forms run the same
MFMA chain — ascending k in the column update, ascending column of X in the product with inv(L_kk)^T (strip_item,
k_tilegemm.hip) — so all seven blocks must be equal BIT FOR BIT; a tolerance has no place here.
tests/test_gpu_tile_build_parent_bits.py pins the call at one and two tile columns (n = 128, 129, 200).  Here, with F = 5,
scalar and vector doT:
  n = 300  three tile columns: column 2's K loop spans two tiles of both operands' row strips;
  n = 513  five tile columns with one live row in the last.
tests/golden/ld_solve_parent_hashes.json holds the parent commit's hash and the SHA-256 of every block the parent returned on an
MI355X, recorded twice in one process and the same both times."""
import json
import os

import pytest

from test_gpu_tile_build_parent_bits import LD_BLOCKS, _digest, _ld

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ld_solve_parent_hashes.json")
CASES = {f"ld_{form}_n{n}_F5": (n, 5, form, 520 + 10 * i + j)
         for i, form in enumerate(("scalar", "vector")) for j, n in enumerate((300, 513))}


def compute(gp, case_id):
    return {k: _digest(a) for k, a in zip(LD_BLOCKS, _ld(gp, *CASES[case_id]))}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", list(CASES))
def test_blocks_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    assert len(CASES) == 4
    assert sorted(recorded["hashes"]) == sorted(CASES)
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in CASES:
        assert sorted(recorded["hashes"][cid]) == sorted(LD_BLOCKS), cid
