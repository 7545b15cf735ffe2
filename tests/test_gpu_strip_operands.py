"""The strip work item (strip_item, k_tilegemm.hip: column update + panel product of one tile) against results recorded BEFORE
its operand staging was changed.  The change moves the A operand from LDS into registers and interleaves the two 16-row blocks of
a wave's strip; rows are independent in both phases, so every output element keeps its MFMA chain and its order: every output
must be equal BIT FOR BIT.  tests/golden/strip_item_parent_hashes.json holds the SHA-256 of meanSATE, varSATE and MeanITE that the
parent commit returned on an MI355X for the seeded cases below: 2, 5, 8, 9 and 32 tiles per side and one size with a partial last
tile (N = 700), through the persistent task launch and through the per-column / panel schedule, with L = 1 (the augmented row
rides with the diagonal tasks) and L = 40 (the augmented row as a tile row of its own), and one unit-B case with seeded draws
(the W = D L^-T solve runs on the same work item).  The work replaced: src/likelihood.jl:42-43, src/estimation.jl:46."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strip_item_parent_hashes.json")
SIZES = (256, 640, 1024, 1152, 4096, 700)          # 2, 5, 8, 9, 32 tiles per side; 6 tiles with a partial last one
LEVELS = (1, 40)
SCHEDULES = (("tasks", 32), ("columns", 0))        # gpslc_set_task_schedule max_tiles


def _samples(n):
    return 3 if n <= 1152 else 2


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _predict_case(gp, n, L, tiles):
    """-> (hashes of meanSATE, varSATE, MeanITE; number of persistent launches that really ran)"""
    c = cases.make_case(n, "UX", False, S=_samples(n), seed=7 * n + L)
    doT = np.linspace(-0.6, 0.8, L)
    g = cases.gpslc_object(gp, c)
    g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)      # HIP-event records: which schedule really ran
    g._ctx.set_data(g.X, g.T, g.Y)
    g.ctx().set_task_schedule(2, tiles, 1, 0)
    g.ctx().profile_reset()
    ms, vs, mi = gp.predict(g, doT, want_mean_ite=True)
    launches = g.ctx().profile_get(4)[0]
    return {"meanSATE": _digest(ms), "varSATE": _digest(vs), "MeanITE": _digest(mi)}, launches


def _unit_b_case(gp, tiles):
    c = cases.make_case(640, "UX", False, S=3, seed=77)
    g = cases.gpslc_object(gp, c)
    g.ctx().set_task_schedule(2, tiles, 1, 0)
    ms, vs, mi, dr = gp.predict(g, [0.1, 0.6], want_mean_ite=True, spp=3, seed=5, want_draws=True)
    return {"meanSATE": _digest(ms), "varSATE": _digest(vs), "MeanITE": _digest(mi), "draws": _digest(dr)}


def case_ids():
    ids = [f"n{n}_L{L}_{name}" for n in SIZES for L in LEVELS for name, _ in SCHEDULES]
    return ids + [f"unitb_n640_{name}" for name, _ in SCHEDULES]


def compute(gp, case_id):
    parts = case_id.split("_")
    tiles = dict(SCHEDULES)[parts[-1]]
    if parts[0] == "unitb":
        return _unit_b_case(gp, tiles), None
    return _predict_case(gp, int(parts[0][1:]), int(parts[1][1:]), tiles)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    got, launches = compute(gp, case_id)
    if launches is not None:
        assert (launches > 0) == case_id.endswith("_tasks"), (case_id, launches)     # the schedule asked for is the one that ran
    assert got == recorded["hashes"][case_id], case_id


def test_both_schedules_were_recorded_equal(recorded):
    """The fixture itself: the parent returned the same bits from the task launch and from the per-column schedule."""
    h = recorded["hashes"]
    assert sorted(h) == sorted(case_ids())
    for cid in case_ids():
        if cid.endswith("_tasks"):
            assert h[cid] == h[cid[:-len("tasks")] + "columns"], cid
