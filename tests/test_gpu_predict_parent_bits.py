"""Every prediction entry point against results recorded BEFORE the prediction path's plumbing was folded together: one
request struct through the host front end (request.h), one SampleGrid inside the launch-argument structs (gpslc_internal.h)
and the weighted right-hand sides / epilogue served by the general kernels (k_gram.hip).  None of that reorders a
floating-point operation, so every output must be equal BIT FOR BIT; a tolerance has no place here.
tests/golden/predict_parent_hashes.json holds the parent commit's hash and the SHA-256 of every output array the parent
returned on an MI355X for the seeded cases below: plain levels (L = 2 with MeanITE and seeded draws, L = 40 with the
augmented row as a tile row of its own and the epilogue's 16-block path) under both schedules, the model shapes U / X / T,
an fp32-kernel context, a binary treatment, vector levels, contrasts (one pair with a == b), weighted effects with
L * G = 6, 18 (the 16-block epilogue path), 37 and 136 rows (two augmented tile rows), the three ITEDistributions forms,
a call sharded over two contexts, the other callers of run_predict (yLogpdf, nodesLogpdf, nodesDraw at n = 700) and the
likelihood blocks with a scalar and a vector doT.  Every output was repeatable on the parent (two runs of `compute` in one
process gave the same hashes), so none is left out.
The fp32-kernel case (plain_fp32) is NOT the parent's bits any more: the mixed-precision mode now centres every feature column
and T on its first element in fp64 before the fp32 rounding (centred_value, gpslc_internal.h), which changes its
results by design.  Its entry (the fixture's "fp32_entries" note names it) holds the bits of the commit that introduced the
centring, recorded twice in one process on an MI355X and equal both times; every other entry passed unchanged on that commit.
It stays a bit-for-bit assertion.  The work replaced: src/estimation.jl:36-163, src/likelihood.jl:8-174."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_parent_hashes.json")
SCHEDULES = (("tasks", 32), ("columns", 0))        # gpslc_set_task_schedule max_tiles
WEIGHTED = ((2, False), (2, True), (6, False), (12, False), (45, False))      # (L, with a baseline), G = 3
SHARD_PAIR = ("sharded_L2", "plain_L2_columns")    # the same call over two contexts and over one


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _named(names, arrays):
    return {k: _digest(a) for k, a in zip(names, arrays)}


OUT4 = ("meanSATE", "varSATE", "MeanITE", "draws")


def _obj(gp, n, shape="UX", binary_t=False, S=3, seed=0, tiles=None, **kw):
    g = cases.gpslc_object(gp, cases.make_case(n, shape, binary_t, S=S, seed=seed), **kw)
    if tiles is not None:
        g.ctx().set_task_schedule(2, tiles, 1, 0)
    return g


def _plain(gp, L, tiles):
    if L == 2:
        g = _obj(gp, 700, S=3, seed=11, tiles=tiles)
        return _named(OUT4, gp.predict(g, [0.1, 0.6], want_mean_ite=True, spp=3, seed=5, want_draws=True))
    g = _obj(gp, 1152, S=2, seed=12, tiles=tiles)
    return _named(OUT4, gp.predict(g, np.linspace(-0.6, 0.8, L), want_mean_ite=True))


def _sharded(gp):
    g = _obj(gp, 700, S=3, seed=11)
    return _named(OUT4, gp.predict(g, [0.1, 0.6], want_mean_ite=True, spp=3, seed=5, want_draws=True, devices=[0, 0]))


def _variant(gp, what):
    if what in cases.SHAPES:
        g = _obj(gp, 200, shape=what, S=3, seed=21)
    elif what == "fp32":
        g = _obj(gp, 200, S=3, seed=22, fp32_kernel=True)
    else:
        g = _obj(gp, 200, binary_t=True, S=3, seed=23)
    doT = [0.0, 1.0] if what == "binary" else [-0.3, 0.7]
    return _named(OUT4, gp.predict(g, doT, want_mean_ite=True))


def _vector_levels(n, seed):
    return np.random.Generator(np.random.Philox(seed)).uniform(-1.0, 1.0, (2, n))


def _vec(gp):
    g = _obj(gp, 700, S=3, seed=31)
    return _named(OUT4, gp.predict(g, _vector_levels(700, 310), want_mean_ite=True, spp=3, seed=6, want_draws=True))


def _contrast(gp):
    g = _obj(gp, 700, S=3, seed=32)
    return _named(OUT4, gp.predict(g, [0.1, 0.6], baseline=[0.1, -0.3], want_mean_ite=True, spp=3, seed=7,
                                   want_draws=True))


def _weighted(gp, L, with_base):
    n = 1152 if L == 45 else 700
    g = _obj(gp, n, S=2, seed=40 + L + with_base)
    rng = np.random.Generator(np.random.Philox(400 + L))
    W = np.stack([np.full(n, 1.0 / n), rng.uniform(-1.0, 1.0, n) / n, (np.arange(n) % 3 == 0) / float(len(range(0, n, 3)))])
    base = np.linspace(0.5, -0.5, L) if with_base else None
    return _named(OUT4, gp.predict(g, np.linspace(-0.6, 0.8, L), baseline=base, weights=W, want_mean_ite=True))


def _ite_distributions(gp, form):
    g = _obj(gp, 200, S=2, seed=51)
    if form == "vec":
        out = gp.ITEDistributions(g, _vector_levels(200, 510)[0])
    else:
        out = gp.ITEDistributions(g, 0.4, baseline=-0.2 if form == "contrast" else None)
    return _named(("MeanITEs", "CovITEs"), out)


def _ylogpdf(gp):
    return {"logpdf": _digest(gp.yLogpdf(_obj(gp, 700, S=3, seed=61)))}


def _nodes(gp):
    """Three nodes of unequal nF (2, 5 and 6 feature columns) beyond the single-workgroup kernels."""
    n = 700
    rng = np.random.Generator(np.random.Philox(62))
    U, X, T = rng.standard_normal((n, 2)), rng.standard_normal((n, 3)), rng.standard_normal(n)
    ls = 1.0 + rng.random(6)
    tg = rng.standard_normal((n, 3))
    nodes = [(U, ls[:2], 1.1, 0.7, tg[:, 0]),
             (np.hstack([U, X]), ls[:5], 1.2, 0.6, tg[:, 1]),
             (np.hstack([U, X, T[:, None]]), ls, 0.9, 0.5, tg[:, 2])]
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.nodesLogpdf(nodes, ctx)), "draw": _digest(gp.nodesDraw(nodes, ctx))}


def _likelihood(gp, form):
    c = cases.make_case(200, "UX", False, S=1, seed=71)
    doT = _vector_levels(200, 710)[0] if form == "vec" else 0.4
    out = gp.likelihoodDistribution(c["uyLS"][:, 0], c["xyLS"][:, 0], c["tyLS"][0], c["yNoise"][0], c["yScale"][0],
                                    c["U"][:, :, 0], c["X"], c["T"], c["Y"], doT)
    return _named(("CovWW", "CovWWs", "CovWWp", "CovC11", "CovC12", "CovC21", "CovC22"), out[1:])


def _weighted_id(L, with_base):
    return f"weighted_G3_L{L}" + ("_base" if with_base else "")


CASES = {}
for _L in (2, 40):
    for _name, _tiles in SCHEDULES:
        CASES[f"plain_L{_L}_{_name}"] = (_plain, _L, _tiles)
for _w in ("U", "X", "T", "fp32", "binary"):
    CASES[f"plain_{_w}"] = (_variant, _w)
CASES["vector_L2"] = (_vec,)
CASES["contrast_L2"] = (_contrast,)
for _L, _b in WEIGHTED:
    CASES[_weighted_id(_L, _b)] = (_weighted, _L, _b)
for _f in ("plain", "vec", "contrast"):
    CASES[f"itedist_{_f}"] = (_ite_distributions, _f)
CASES[SHARD_PAIR[0]] = (_sharded,)
CASES["ylogpdf_n700"] = (_ylogpdf,)
CASES["nodes_n700"] = (_nodes,)
for _f in ("scalar", "vec"):
    CASES[f"likelihood_{_f}"] = (_likelihood, _f)


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
    """Bit for bit against the fixture: the parent's bits, except plain_fp32, which holds the bits of the commit that centred the
    fp32 mode's features (module docstring)."""
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_sharded_call_was_recorded_equal_to_the_single_context(recorded):
    """The fixture itself: every case is there, and the parent returned the same bits from two contexts as from one."""
    h = recorded["hashes"]
    assert sorted(h) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert h[SHARD_PAIR[0]] == h[SHARD_PAIR[1]]
    for L in (2, 40):                                  # and, like the strip fixture, from both schedules
        assert h[f"plain_L{L}_tasks"] == h[f"plain_L{L}_columns"], L
