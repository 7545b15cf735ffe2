"""The factorisation path against results recorded BEFORE its settled A/B switches were retired ("Retired
switches"): factor_panels with one path per column, w_solve as one loop of fused launches, the tile product and the fused strip
kernel without their queue-less and non-temporal bodies.  Removing a side that never ran reorders no floating-point operation,
so every output must be equal BIT FOR BIT; a tolerance has no place here.
tests/golden/factor_parent_hashes.json holds the parent commit's hash and the SHA-256 of every output array the parent returned
on an MI355X for the seeded cases below, which reach what tests/golden/predict_parent_hashes.json and
strip_item_parent_hashes.json do not: trailing updates of 9 and 1 tile rows plus the augmented row under the per-column
schedule (N = 2176 = 17 tiles with the default panel width, so the L2-blocked tile order and a ticket queue that turns over are
in use), the same schedule at N = 1152 with panels of 4 tiles on two streams, unit B at N = 700 with L = 3 (w_solve,
factor_robust, the draw kernels: ITEDistributions and seeded draws) and the tiled robust factor behind mvnLogpdf / mvnDraw
at n = 700.  Every output was recorded twice on the parent, in two contexts of one process, and was the same both times, so
none is left out.  The measurement build with no switch set must return the product library's bits.
The work replaced: src/estimation.jl:36-163, src/model_likelihood.jl:4-10."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "factor_parent_hashes.json")
COLUMNS = (2, 0, 1, 0)                             # gpslc_set_task_schedule: max_tiles = 0, the per-column schedule
DIAG_CASE = "predict_n1152_panel4_streams2"
OUT4 = ("meanSATE", "varSATE", "MeanITE", "draws")


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _named(names, arrays):
    return {k: _digest(a) for k, a in zip(names, arrays)}


def _predict_columns(gp, n, seed, tuning=None):
    g = cases.gpslc_object(gp, cases.make_case(n, "UX", False, S=2, seed=seed))
    g.ctx().set_task_schedule(*COLUMNS)
    if tuning is not None:
        g.ctx().set_tuning(*tuning)                # max_batch, panel_tiles, n_streams
    return _named(OUT4, gp.predict(g, [0.1, 0.6], want_mean_ite=True))


def _unit_b(gp):
    g = cases.gpslc_object(gp, cases.make_case(700, "UX", False, S=2, seed=83))
    out = _named(("MeanITEs", "CovITEs"), gp.ITEDistributions(g, 0.4))
    out.update(_named(OUT4, gp.predict(g, [-0.5, 0.1, 0.6], want_mean_ite=True, spp=3, seed=9, want_draws=True)))
    return out


def _unit_b_deep(gp):
    """34 tiles per side: w_solve's K loop is deeper than 32 tiles in its last column, and the factorisations run four panels."""
    g = cases.gpslc_object(gp, cases.make_case(4352, "UX", False, S=1, seed=85))
    return _named(OUT4, gp.predict(g, [0.3], want_mean_ite=True, spp=2, seed=3, want_draws=True))


def _mvn(gp):
    """cov = 1 / (1 + |t_i - t_j|) + 0.01 I (positive definite by Polya's criterion), built from exactly rounded operations
    only, so the host forms the same bits everywhere."""
    n, S = 700, 3
    rng = np.random.Generator(np.random.Philox(84))
    t = 4.0 * rng.random(n)
    cov = 1.0 / (1.0 + np.abs(t[:, None] - t[None, :])) + 0.01 * np.eye(n)
    x, z = rng.standard_normal((n, S)), rng.standard_normal((n, S))
    cs = np.array([0.5, 1.0, 2.25])
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.mvnLogpdf(cov, x, covscale=cs, ctx=ctx)),
            "draw": _digest(gp.mvnDraw(cov, z, covscale=cs, ctx=ctx))}


CASES = {
    "predict_n2176_columns": (_predict_columns, 2176, 81),
    DIAG_CASE: (_predict_columns, 1152, 82, (0, 4, 2)),
    "unit_b_n700_L3": (_unit_b,),
    "unit_b_n4352_draws": (_unit_b_deep,),
    "mvn_n700": (_mvn,),
}


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
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, with every output, and the parent's second run gave the first one's bits."""
    assert sorted(recorded["hashes"]) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in ("predict_n2176_columns", DIAG_CASE):
        assert sorted(recorded["hashes"][cid]) == sorted(OUT4[:3])
    assert sorted(recorded["hashes"]["unit_b_n700_L3"]) == sorted(OUT4 + ("MeanITEs", "CovITEs"))
    assert sorted(recorded["hashes"]["unit_b_n4352_draws"]) == sorted(OUT4)
    assert sorted(recorded["hashes"]["mvn_n700"]) == ["draw", "logpdf"]


def test_measurement_build_without_switches_equals_the_product_library(recorded):
    """libgpslc_hip_diag.so reads its GPSLC_* switches once per process, so it runs in a fresh one with none of them set: the
    kept instruments are all off by default and the build must then compute what the product library computes."""
    diag = os.path.join(ROOT, "causalgpslc.jl_amd", "csrc", "libgpslc_hip_diag.so")
    assert os.path.exists(diag), "measurement build not present (make -C causalgpslc.jl_amd/csrc diag)"
    code = (
        "import sys, json\n"
        f"sys.path[:0] = [{ROOT!r}, {HERE!r}, {os.path.join(ROOT, 'oracle')!r}]\n"
        "import causalgpslc_jl_amd as gp, test_gpu_factor_parent_bits as t\n"
        "gp._lib.LIB_PATH = gp._lib.LIB_PATH.replace('libgpslc_hip.so', 'libgpslc_hip_diag.so')\n"
        f"print('HASHES', json.dumps(t.compute(gp, {DIAG_CASE!r})))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("GPSLC_")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("HASHES ")][-1]
    assert json.loads(line[len("HASHES "):]) == recorded["hashes"][DIAG_CASE]
