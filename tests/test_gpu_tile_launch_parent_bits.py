"""The launches of the tile-product kernels against results recorded BEFORE their descriptions moved into builders
(causalgpslc.jl_amd/csrc/tile_launch.h): the same launches with the same fields reorder no floating-point operation, so every
output must be equal BIT FOR BIT, and the profiler's launch counts and flop totals, which the host computes from the launch
descriptions alone, must be the same numbers.  A tolerance has no place here.
tests/golden/tile_launch_parent_hashes.json holds the parent commit's hash and what the parent returned on an MI355X for what
the other parent-bit fixtures do not pin:
  * mvnLogpdf at n = 641 with S = 130 vectors: two augmented tile rows, so the rectangle updates of the tiled forward solve run
    with no short row (short_rows == 0), with and without covscale — covariance as _mvn of test_gpu_factor_parent_bits.py;
  * per kernel class of gpslc_profile_get_class, the launch count and the flop total (the hex of the double) of a profiled
    context after predict at n = 700 with S = 2, three levels and draws; predict at n = 1152 under the per-column schedule with
    panels of 4 tiles on two streams; ITEDistributions at n = 700.  Times are not compared.
Every case was recorded twice on the parent in one process and was the same both times.
The work replaced: src/estimation.jl:36-163, src/model_likelihood.jl:4-10."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_launch_parent_hashes.json")
CLASSES = range(5)          # include/gpslc_hip.h: trailing updates, fused strips, draws, the ITE-covariance path, task launches


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _mvn_two_aug_rows(gp):
    """cov = 1 / (1 + |t_i - t_j|) + 0.01 I from exactly rounded operations only (the same bits on every host)"""
    n, S = 641, 130
    rng = np.random.Generator(np.random.Philox(86))
    t = 4.0 * rng.random(n)
    cov = 1.0 / (1.0 + np.abs(t[:, None] - t[None, :])) + 0.01 * np.eye(n)
    x = rng.standard_normal((n, S))
    cs = 0.25 * (1 + np.arange(S) % 9)          # exact in binary
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.mvnLogpdf(cov, x, ctx=ctx)), "logpdf_covscale": _digest(gp.mvnLogpdf(cov, x, covscale=cs, ctx=ctx))}


def _profiled(gp, n, seed, run, schedule=None, tuning=None):
    g = cases.gpslc_object(gp, cases.make_case(n, "UX", False, S=2, seed=seed))
    g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)
    g._ctx.set_data(g.X, g.T, g.Y)
    if schedule is not None:
        g.ctx().set_task_schedule(*schedule)
    if tuning is not None:
        g.ctx().set_tuning(*tuning)
    g.ctx().profile_reset()
    run(g)
    out = {}
    for k in CLASSES:
        launches, _ms, flop = g.ctx().profile_get(k)
        out[f"class{k}"] = [int(launches), float(flop).hex()]
    return out


def _profile_predict_draws(gp):
    return _profiled(gp, 700, 87, lambda g: gp.predict(g, [-0.5, 0.1, 0.6], want_mean_ite=True, spp=3, seed=9, want_draws=True))


def _profile_predict_columns(gp):
    return _profiled(gp, 1152, 88, lambda g: gp.predict(g, [0.1, 0.6], want_mean_ite=True), schedule=(2, 0, 1, 0), tuning=(0, 4, 2))


def _profile_ite_distributions(gp):
    return _profiled(gp, 700, 89, lambda g: gp.ITEDistributions(g, 0.4))


CASES = {
    "mvn_logpdf_n641_S130": _mvn_two_aug_rows,
    "profile_predict_n700_L3_draws": _profile_predict_draws,
    "profile_predict_n1152_columns_panel4_streams2": _profile_predict_columns,
    "profile_ite_distributions_n700": _profile_ite_distributions,
}


def compute(gp, case_id):
    return CASES[case_id](gp)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", list(CASES))
def test_outputs_and_profiler_totals_equal_the_parents(gp, recorded, case_id):
    got = compute(gp, case_id)
    print(case_id, json.dumps(got))
    assert got == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, the parent's second run gave the first one's numbers, and the profiled calls
    did launch tile kernels (a fixture of zeros would pin nothing)."""
    assert sorted(recorded["hashes"]) == sorted(CASES)
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    assert sorted(recorded["hashes"]["mvn_logpdf_n641_S130"]) == ["logpdf", "logpdf_covscale"]
    for cid in CASES:
        if cid.startswith("profile_"):
            h = recorded["hashes"][cid]
            assert sorted(h) == [f"class{k}" for k in CLASSES]
            assert sum(v[0] for v in h.values()) > 0 and any(float.fromhex(v[1]) > 0 for v in h.values()), cid
    # the per-column schedule launches no task kernel; unit B (ITEDistributions) runs the pair workspaces' launches
    assert recorded["hashes"]["profile_predict_n1152_columns_panel4_streams2"]["class4"][0] == 0
    assert recorded["hashes"]["profile_predict_n1152_columns_panel4_streams2"]["class0"][0] > 0
    assert recorded["hashes"]["profile_ite_distributions_n700"]["class3"][0] > 0
