"""The node-score entry points (gpslc_y_logpdf, gpslc_gp_logpdf, gpslc_nodes_logpdf, gpslc_nodes_draw, gpslc_mvn_logpdf,
gpslc_mvn_draw) against results recorded BEFORE their host side was folded together: one constructor per kind of node view,
one body for the fused node calls, one tiled score, one MVN prologue, one zero-mean node draw (api_score.hip).  None of that
touches a kernel or reorders a floating-point operation, so every output must be equal BIT FOR BIT; a tolerance has no place
here.  tests/golden/node_parent_hashes.json holds the parent commit's hash and the SHA-256 of every output the parent returned
on an MI355X for the seeded cases below, at the smallest sizes that reach each path: n = 150 (the LDS-resident kernel), 400
(the left-looking kernel) and 641 (the first size past both: the tiled path).  test_gpu_predict_parent_bits.py already pins
yLogpdf, nodesLogpdf and nodesDraw at n = 700; here are six nodes of unequal feature counts in one launch (more than the
kernel takes inline), the four forms of gpLogpdf, yLogpdf with its overrides, the MVN score and draw with a covariance handed
over and re-used (through either call), failing nodes and covariances with their info codes, and an fp32-kernel context
(which sends a small n down the tiled path).  Every output was repeatable on the parent (two runs of `compute` in one process
gave the same hashes), so none is left out.
The fp32-kernel case (ylogpdf_n150_fp32) is NOT the parent's bits any more: the mixed-precision mode now centres every feature
column and T on its first element in fp64 before the fp32 rounding (centred_value, gpslc_internal.h), which changes
its Gram matrix by design.  Its entry (the fixture's "fp32_entries" note names it) holds the bits of the commit that introduced
the centring, recorded twice in one process on an MI355X and equal both times; every other entry passed unchanged on that commit.
It stays a bit-for-bit assertion.  The work replaced: src/model_likelihood.jl:4-120, src/inference.jl:48-54."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_parent_hashes.json")
NODE_NF = (0, 2, 2, 5, 6, 8)                    # six nodes: more than SMALL_INLINE_NODES = 4 descriptors
GP_FORMS = ("own_F", "shared_F", "shared_target", "no_F")
MVN_SAME = ("logpdf", "logpdf_cached", "logpdf_after_draw_hand_over")      # one covariance, three ways to hand it over


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _nodes(gp, n):
    rng = _rng(7000 + n)
    F = rng.standard_normal((n, max(NODE_NF)))
    nodes = []
    for i, nF in enumerate(NODE_NF):
        Fi = None if nF == 0 else np.asfortranarray(F[:, i % 2:i % 2 + nF] if nF < max(NODE_NF) else F)
        nodes.append((Fi, 1.0 + rng.random(nF), 0.8 + 0.1 * i, 0.4 + 0.05 * i, rng.standard_normal(n)))
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.nodesLogpdf(nodes, ctx)), "draw": _digest(gp.nodesDraw(nodes, ctx))}


def _gp_logpdf(gp, n, form):
    S = 3
    rng = _rng(7100 + n)
    F = rng.standard_normal((n, 3, S))
    ls = 1.0 + rng.random((3, S))
    scale, noise = 0.9 + rng.random(S), 0.3 + rng.random(S)
    tg = rng.standard_normal((n, S))
    if form == "own_F":
        out = gp.gpLogpdf(F, ls, scale, noise, tg)
    elif form == "shared_F":
        out = gp.gpLogpdf(F[:, :, 0], ls, scale, noise, tg)
    elif form == "shared_target":
        out = gp.gpLogpdf(F, ls, scale, noise, tg[:, 0])
    else:
        out = gp.gpLogpdf(None, None, scale, noise, tg)
    return {"logpdf": _digest(out)}


def _y_logpdf(gp, n, what):
    c = cases.make_case(n, "UX", False, S=3, seed=72)
    g = cases.gpslc_object(gp, c, **({"fp32_kernel": True} if what == "fp32" else {}))
    rng = _rng(7200 + n)
    Xo = rng.standard_normal(c["X"].shape) if what in ("X_override", "both") else None
    Yo = rng.standard_normal(n) if what in ("Y_override", "both") else None
    return {"logpdf": _digest(gp.yLogpdf(g, X_override=Xo, Y_override=Yo))}


def _block_cov(n):
    obj = np.repeat(np.arange((n + 24) // 25), 25)[:n]
    return (obj[:, None] == obj[None, :]).astype(float) + 1e-6 * np.eye(n)


def _mvn(gp, n):
    rng = _rng(7300 + n)
    Sig = _block_cov(n)
    x = np.linalg.cholesky(Sig) @ rng.standard_normal((n, 3))
    z = rng.standard_normal((n, 3))
    cs = np.array([0.7, 1.9, 4.0])
    out = {}
    ctx = gp.Context(n, 0, 0)
    out["logpdf"] = _digest(gp.mvnLogpdf(Sig, x, covscale=cs, ctx=ctx))
    out["logpdf_cached"] = _digest(gp.mvnLogpdf(None, x, covscale=cs, ctx=ctx))
    out["draw_cached"] = _digest(gp.mvnDraw(None, z, covscale=cs, ctx=ctx))
    out["logpdf_no_covscale"] = _digest(gp.mvnLogpdf(None, x, ctx=ctx))
    ctx2 = gp.Context(n, 0, 0)
    out["draw"] = _digest(gp.mvnDraw(Sig, z, covscale=cs, ctx=ctx2))
    out["logpdf_after_draw_hand_over"] = _digest(gp.mvnLogpdf(None, x, covscale=cs, ctx=ctx2))
    out["draw_no_covscale"] = _digest(gp.mvnDraw(None, z, ctx=ctx2))
    return out


def _failing_node(gp):
    n = 150
    rng = _rng(7400)
    F = rng.standard_normal((n, 4))
    nodes = [(F[:, :2], [1.2, 1.7], 1.1, 0.7, rng.standard_normal(n)),
             (F, [1.2, 1.7, 0.9, 1.4], 1.3, -5.0, rng.standard_normal(n)),          # K = 1.3 exp(...) - 5 I: not positive definite
             (F[:, 1:], [1.1, 1.3, 1.6], 0.9, 0.5, rng.standard_normal(n))]
    ctx = gp.Context(n, 0, 0)
    lp = gp.nodesLogpdf(nodes, ctx, fail_value=-np.inf)
    return {"logpdf": _digest(lp), "last_info": _digest(ctx.last_info(3))}


def _failing_cov(gp):
    n = 150
    Sig = _block_cov(n)
    Sig[7, 7] = -1.0                                  # the pivot of row 8 is negative
    rng = _rng(7500)
    ctx = gp.Context(n, 0, 0)

    def outcome(fn, *a, **kw):
        try:
            return "returned " + _digest(fn(*a, **kw))
        except gp.PosDefException as e:
            return f"PosDefException({e.info})"
    return {"mvnLogpdf_S0": outcome(gp.mvnLogpdf, Sig, np.zeros((n, 0)), ctx=ctx),
            "mvnLogpdf_S2": outcome(gp.mvnLogpdf, Sig, rng.standard_normal((n, 2)), ctx=ctx),
            "mvnDraw_S0": outcome(gp.mvnDraw, Sig, np.zeros((n, 0)), ctx=ctx)}


CASES = {}
for _n in (150, 400):
    CASES[f"nodes_n{_n}"] = (_nodes, _n)
for _n in (150, 641):
    for _f in GP_FORMS:
        CASES[f"gplogpdf_n{_n}_{_f}"] = (_gp_logpdf, _n, _f)
for _w in ("plain", "X_override", "Y_override"):
    CASES[f"ylogpdf_n150_{_w}"] = (_y_logpdf, 150, _w)
CASES["ylogpdf_n641_both"] = (_y_logpdf, 641, "both")
for _n in (150, 400, 641):                       # 641: the tiled solve and the cached factor on the draw kernel
    CASES[f"mvn_n{_n}"] = (_mvn, _n)
CASES["failing_node_n150"] = (_failing_node,)
CASES["failing_cov_n150"] = (_failing_cov,)
CASES["ylogpdf_n150_fp32"] = (_y_logpdf, 150, "fp32")


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
def test_node_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    """Bit for bit against the fixture: the parent's bits, except ylogpdf_n150_fp32, which holds the bits of the commit that
    centred the fp32 mode's features (module docstring)."""
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_fixture_holds_exactly_the_cases_and_a_handed_over_covariance_scores_the_same(recorded):
    """The fixture itself: every case is there, and the parent scored a covariance the same whether the call handed it over,
    re-used it (cov = NULL directly afterwards) or re-used one that gpslc_mvn_draw had been handed."""
    h = recorded["hashes"]
    assert sorted(h) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    for n in (150, 400, 641):
        m = h[f"mvn_n{n}"]
        assert m[MVN_SAME[0]] == m[MVN_SAME[1]] == m[MVN_SAME[2]], n
        assert m["draw"] == m["draw_cached"], n
