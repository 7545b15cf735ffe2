"""The single-workgroup node kernels (csrc/k_small.hip: the LDS-resident score, its gradient twin and the left-looking kernel for
176 < n <= 640) against results recorded BEFORE their layouts moved into csrc/sm_layout.h and their repeated pieces into
csrc/sm_blocks.h.  That change touches no arithmetic, no operation order, no launch shape and no path choice, so every output
must be equal BIT FOR BIT; a tolerance has no place here.  tests/golden/small_kernels_parent_hashes.json holds the parent
commit's hash and the SHA-256 of every output the parent returned on an MI355X for the seeded cases below.  These kernels have
no atomics and fixed summation orders: every case was repeatable on the parent (two runs of `compute` in one process gave the
same hashes), so none is left out.  Every call is one launch of at most six nodes, at the smallest shapes that reach each code
path (test_gpu_node_parent_bits.py already pins n = 150 and the two-column-image variant of the left-looking kernel at n = 400):

  score and draw, six nodes of nF = (0, 2, 2, 5, 6, 8) — more than the four inline descriptors
    LDS-resident   n = 1, 16 (one block, no loop), 17 (two blocks: the first look-ahead step), 33 (three blocks: carriers and
                   updaters split), 176 (the largest size)
    left-looking   n = 177 (shared operand row), 544 (features resident, one column image), 640 (the limit)
  one node of nF = 32 at n = 416: the left-looking variant with none of the three; at n = 160: the LDS-resident score's limit
  dense-covariance nodes (mvnLogpdf, mvnDraw with covscale) at n = 17, 177, 640
  gradient (all five outputs and the score): the six-node mix at n = 3, 16, 17, 48; one node each at the limits (n, nF) =
    (176, 7), (160, 17), (128, 32) and at (150, 0); three nodes at n = 48 with the middle one not positive definite (NaN for it,
    last_info recorded).
The work replaced: src/model_likelihood.jl:4-120, src/inference.jl:21-56."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_kernels_parent_hashes.json")
NODE_NF = (0, 2, 2, 5, 6, 8)                    # six nodes: more than SMALL_INLINE_NODES = 4 descriptors
SCORE_N = (1, 16, 17, 33, 176, 177, 544, 640)
WIDE = ((416, 32), (160, 32))                   # one node: the left-looking variant `none`, the LDS-resident score's limit
MVN_N = (17, 177, 640)
GRAD_MIX_N = (3, 16, 17, 48)
GRAD_ONE = ((176, 7), (160, 17), (128, 32), (150, 0))
GRAD_OUT = ("dF", "dls", "dscale", "dnoise", "dtarget", "logpdf")


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _make_nodes(n, widths, seed):
    rng = _rng(seed)
    F = rng.standard_normal((n, max(max(widths), 1)))
    nodes = []
    for i, nF in enumerate(widths):
        o = i % 2 if nF + 1 < F.shape[1] else 0
        Fi = None if nF == 0 else np.asfortranarray(F[:, o:o + nF])
        nodes.append((Fi, 1.0 + rng.random(nF), 0.8 + 0.1 * i, 0.4 + 0.05 * i, rng.standard_normal(n)))
    return nodes


def _score_draw(gp, n, widths, seed):
    nodes = _make_nodes(n, widths, seed)
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.nodesLogpdf(nodes, ctx)), "draw": _digest(gp.nodesDraw(nodes, ctx))}


def _mvn(gp, n):
    rng = _rng(8300 + n)
    obj = np.repeat(np.arange((n + 24) // 25), 25)[:n]
    Sig = (obj[:, None] == obj[None, :]).astype(float) + 1e-3 * np.eye(n)
    x = np.linalg.cholesky(Sig) @ rng.standard_normal((n, 3))
    z = rng.standard_normal((n, 3))
    cs = np.array([0.7, 1.9, 4.0])
    ctx = gp.Context(n, 0, 0)
    return {"logpdf": _digest(gp.mvnLogpdf(Sig, x, covscale=cs, ctx=ctx)),
            "draw": _digest(gp.mvnDraw(None, z, covscale=cs, ctx=ctx))}


def _grad_digests(ctx, nodes):
    st, out = ctx.nodes_logpdf_grad(nodes, GRAD_OUT)
    res = {k: _digest(out[k]) for k in GRAD_OUT}
    res["status"] = int(st)
    return res


def _grad(gp, n, widths, seed):
    return _grad_digests(gp.Context(n, 0, 0), _make_nodes(n, widths, seed))


def _grad_failing(gp):
    n = 48
    nodes = _make_nodes(n, (2, 4, 3), 8500)
    F, ls, scale, _, tg = nodes[1]
    nodes[1] = (F, ls, scale, -5.0, tg)          # K = scale exp(...) - 5 I: not positive definite
    ctx = gp.Context(n, 0, 0)
    res = _grad_digests(ctx, nodes)
    res["last_info"] = _digest(ctx.last_info(3))
    return res


CASES = {}
for _n in SCORE_N:
    CASES[f"nodes_n{_n}"] = (_score_draw, _n, NODE_NF, 8000 + _n)
for _n, _f in WIDE:
    CASES[f"node_n{_n}_nF{_f}"] = (_score_draw, _n, (_f,), 8100 + _n)
for _n in MVN_N:
    CASES[f"mvn_n{_n}"] = (_mvn, _n)
for _n in GRAD_MIX_N:
    CASES[f"grad_nodes_n{_n}"] = (_grad, _n, NODE_NF, 8400 + _n)
for _n, _f in GRAD_ONE:
    CASES[f"grad_n{_n}_nF{_f}"] = (_grad, _n, (_f,), 8450 + _n)
CASES["grad_failing_n48"] = (_grad_failing,)


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
def test_small_kernel_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    """Computed twice in one process: both runs give the same hashes, and they are the parent's."""
    first, second = compute(gp, case_id), compute(gp, case_id)
    assert first == second, case_id
    assert first == recorded["hashes"][case_id], case_id


def test_fixture_holds_exactly_the_cases_and_the_failing_node_is_the_middle_one(recorded):
    h = recorded["hashes"]
    assert sorted(h) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert h["grad_failing_n48"]["status"] > 0
    assert all(h[k]["status"] == 0 for k in h if k.startswith("grad_") and k != "grad_failing_n48")
