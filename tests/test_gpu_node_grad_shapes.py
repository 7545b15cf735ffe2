"""gpslc_nodes_logpdf_grad on an MI355X at the shapes tests/test_gpu_node_grad.py does not reach, against the long-double
restatement (tests/node_grad_restatement.py) with that file's conventions: per element the bound tol * scale,
tol = max(1e-10, 1e-14 cond(A)) and the restatement's scales; the shift identity on dF; `logpdf` = nodesLogpdf bit for bit where the
two calls take one path (a tiled gradient call of a few nodes stands beside a score on the single-workgroup kernels: there within
tol |logpdf|); the path asserted from profile classes 0, 1 and 4 wherever n > 128; last_info all zero.  The inputs are tests/node_grad_cases.py's:
every node with features has its lengthscales rescaled to sum_f 1 / ls_f^2 = 0.5 (cond(A) >= 10 from n = 32 on, so that L, W = L^-1
and A^-1 are dense at every width), except the ill-conditioned ones.  tests/test_node_grad_cases.py shows on the CPU that these
inputs see a missing transposed block, an unmasked padding and a wrong set's target by more than 1e6 bounds.

1. Block counts: the single launch at NB = 1 .. 11 blocks of 16 rows, n = 16 NB - 15, 16 NB - 7, 16 NB, three nodes per call of
   widths 0 .. 32 (every width up to 8, 12, 16, and widths >= 9 that are no multiple of 4).
2. The four LDS limits (176, 7), (160, 17), (144, 27), (128, 32): the limit on the single launch, one column more and one row more
   tiled; the limit node through both paths; a mixed call at n = 176.
3. Ill-conditioned nodes (cond(A) 1.3e5 .. 8.5e5) on both paths.
4. Node mode of the tiled pass at 2, 3, 3 and 4 tiles per side (n = 256, 257, 300, 385), a 32-wide node, a shared feature block.
5. Node mode in several chunks and on several streams (gpslc_set_tuning): the bits of the default tuning.
6. Many nodes: 260 at n = 129 beside a 32-wide one (the 260 alone fit the single launch; the 261 take the task launch) and 4097
   at n = 5 (the count > 4096 route: one tile per side).

Measured on one MI355X, worst fraction of the bound per group and path (dtarget is the worst output everywhere but at n = 5; dF <= 1.7e-5):
    block-count sweep   single launch 5.9e-5
    limits              single launch 3.6e-5, tiled 5.9e-5
    ill-conditioned     single launch 4.7e-4, tiled 2.8e-3 (the fp64 restatement itself: 2.4e-3)
    tile counts         tiled 7.8e-5
    chunks              tiled 7.0e-5
    many nodes          task launch 1.2e-5 (the 260 nodes alone on the single launch 1.5e-5); one tile per side 5.8e-6 (the same
                        eight nodes on the single launch 6.1e-6, and not the same bits)
The longest single test takes 0.9 s (test_tile_counts_in_node_mode[385], its references included); the file 6 s."""
import numpy as np
import pytest

import node_grad_cases as nc
import node_grad_restatement as ng

pytestmark = pytest.mark.gpu

OUT = ng.OUTPUTS
WORST = {}


def _traced(ctx, fn):
    """fn() and the launches of the tiled factorisation it recorded: {class: launches} for classes 0, 1 (per-column schedule)
    and 4 (task launch); the single launch records none"""
    ctx.profile_reset()
    out = fn()
    return out, {k: ctx.profile_get(k)[0] for k in (0, 1, 4)}


def _tiled(tr):
    return sum(tr.values()) > 0


def _nodes(keys):
    return [nc.make(k) for k in keys]


def _check(keys, got, what):
    """every node's outputs inside its bound; the shift identity; records the worst fraction of the bound under `what`"""
    worst = 0.0
    for i, (k, g) in enumerate(zip(keys, got)):
        ref, sc, tol, cond = nc.expected(k)
        err = nc.fractions(g, ref, sc)
        print(what, "node", i, k, "cond %.3g" % cond, "error / bound:", {o: v / tol for o, v in err.items()})
        assert max(err.values()) <= tol, (what, i, k, err, tol)
        assert np.all(np.abs(g["dF"].sum(0)) <= tol * np.asarray(sc["dF"].sum(0), dtype=np.float64)), (what, i, "shift identity")
        worst = max(worst, max(err.values()) / tol)
    WORST[what] = max(WORST.get(what, 0.0), worst)
    print("worst fraction of the bound so far:", WORST)
    return worst


def _same_bits(a, b, outs=OUT + ("logpdf",)):
    for o in outs:
        assert np.array_equal(np.asarray(a[o]), np.asarray(b[o]), equal_nan=True), o


def _logpdf_is_nodes_logpdf(gp, ctx, keys, nodes, got, same_path):
    """`logpdf` against gpslc_nodes_logpdf: bit for bit where both calls take the same path.  A tiled gradient call of a few nodes
    stands beside a score on the single-workgroup kernels (n <= 640, up to 512 nodes), which factorises in another order: there
    within tol |logpdf|, the node's own tol (1e-10 is the suite's tolerance between the two paths, tests/test_gpu_path_limits.py)"""
    lp = gp.nodesLogpdf(nodes, ctx)
    mine = np.array([g["logpdf"] for g in got])
    if same_path:
        assert np.array_equal(lp, mine)
    else:
        tol = np.array([nc.expected(k)[2] for k in keys])
        assert np.all(np.abs(lp - mine) <= tol * np.abs(lp)), float(np.max(np.abs(lp - mine) / np.abs(lp)))


def _call(gp, ctx, keys, tiled, what):
    """one call on `ctx`: the path (True: tiled, False: the single launch, None: not asserted — n <= 128, the single launch by the
    code), every node against the reference, logpdf against nodesLogpdf, last_info"""
    nodes = _nodes(keys)
    got, tr = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    if tiled is not None:
        assert ctx.n > 128, "one tile per side leaves no trace in the profile"
        assert _tiled(tr) == tiled, (what, keys, tr)
    assert not ctx.last_info(len(nodes)).any()
    _check(keys, got, what + (", tiled" if tiled else ", single launch"))
    _logpdf_is_nodes_logpdf(gp, ctx, keys, nodes, got, not tiled)
    return got


# ---- 1. every block count of the single launch ------------------------------------------------------------------------------------

@pytest.mark.parametrize("NB", sorted(nc.SWEEP_WIDTHS))
def test_block_counts_on_the_single_launch(gp, NB):
    """NB blocks of 16 rows: the first size of the block count (one live row in the last block), a half-filled and a full last
    block, three nodes of different widths per call.  The waves' loops change shape with NB: a second pass over the diagonal
    blocks and a second accumulator slot from NB = 9 and 10 on, two passes over the packed blocks from NB = 4 on."""
    for n, keys in nc.sweep_keys(NB):
        assert nc.blocks(n) == NB and all(nc.fits_single_launch(n, k[2]) for k in keys)
        nodes = _nodes(keys)
        ctx = gp.Context(n, 0, 0, profile=True)
        got = _call(gp, ctx, keys, False if n > 128 else None, "block-count sweep")
        again = gp.nodesLogpdfGrad(nodes, ctx)
        for a, b in zip(got, again):
            _same_bits(a, b)
        for i in range(len(nodes)):          # each node alone: the bits it has inside the call
            _same_bits(gp.nodesLogpdfGrad(nodes[i:i + 1], ctx)[0], got[i])


# ---- 2. both sides of the four LDS limits ------------------------------------------------------------------------------------------

LIMIT_CALLS = [(s, False if s[0] > 128 else None) for s in nc.LIMIT_SINGLE] + [(s, True) for s in nc.LIMIT_COLUMN + nc.LIMIT_ROW]


@pytest.mark.parametrize("shape,tiled", LIMIT_CALLS, ids=["%dx%d" % s for s, _ in LIMIT_CALLS])
def test_both_sides_of_the_lds_limits(gp, shape, tiled):
    """(176, 7), (160, 17), (144, 27), (128, 32) on the single launch; one column more and one row more tiled.  The path of
    (128, 32) cannot be asserted from the counters: a tiled factorisation of one tile per side records no launch in classes 0, 1
    and 4 either.  That it is the single launch is read from the code (the layout fits: tests/test_node_grad_cases.py) — and
    (129, 32), one row more, is asserted tiled."""
    n, nF = shape
    assert nc.fits_single_launch(n, nF) == (not tiled)
    ctx = gp.Context(n, 0, 0, profile=True)
    _call(gp, ctx, [nc.limit_key(n, nF)], tiled, "limits")


@pytest.mark.parametrize("n,nF", [s for s in nc.LIMIT_SINGLE if s[0] > 128])
def test_the_limit_node_through_both_paths(gp, n, nF):
    """the node at the limit alone (single launch) and beside a node of one column more, which sends the call tiled: within the
    sum of the two bounds"""
    key, wide = nc.limit_key(n, nF), nc.limit_key(n, nF + 1)
    ctx = gp.Context(n, 0, 0, profile=True)
    small = _call(gp, ctx, [key], False, "limits")
    big = _call(gp, ctx, [key, wide], True, "limits")
    _, sc, tol, _ = nc.expected(key)
    for o in OUT:
        assert np.all(np.abs(np.asarray(small[0][o]) - np.asarray(big[0][o])) <= 2 * tol * np.asarray(sc[o], dtype=np.float64)), o


def test_a_mixed_call_at_the_largest_size(gp):
    """n = 176, widths (7, 0, 3): the launch is sized by the widest node and every node builds its own layout — each has the bits
    it has alone"""
    keys = nc.MIXED_176
    nodes = _nodes(keys)
    ctx = gp.Context(176, 0, 0, profile=True)
    got = _call(gp, ctx, keys, False, "limits")
    for i in range(len(nodes)):
        alone, tr = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes[i:i + 1], ctx))
        assert not _tiled(tr)
        _same_bits(alone[0], got[i])


# ---- 3. ill-conditioned nodes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,noise", nc.ILL)
def test_ill_conditioned_nodes(gp, n, noise):
    """three columns at lengthscale 6 with noise 1e-3 or 2e-4: tol = 1e-14 cond(A), the bound's second branch — n = 150 on the
    single launch, n = 200 tiled"""
    key = ("ill", n, noise)
    _, _, tol, cond = nc.expected(key)
    assert 1e4 <= cond <= 1e8 and tol == 1e-14 * cond
    ctx = gp.Context(n, 0, 0, profile=True)
    _call(gp, ctx, [key], n > 176, "ill-conditioned")


# ---- 4. tile counts in node mode ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", nc.TILE_SIZES)
def test_tile_counts_in_node_mode(gp, n):
    """2 tiles per side at an exact multiple (n = 256), 3 with one live row (257) and with 44 (300), 4 with one live row (385):
    widths (3, 0, 8), at n = 257 a 32-wide node too — every feature a column with row and column sums, off-diagonal items with
    K ranges of 1, 2 and 3 tiles, grad_finish_kernel's sum over up to 4 tile columns"""
    ctx = gp.Context(n, 0, 0, profile=True)
    _call(gp, ctx, nc.tile_keys(n), True, "tile counts")


def test_a_shared_feature_block_at_three_tiles(gp):
    """n = 300: three nodes on ONE feature block get one gradient block each; the first of them alone has identical bits"""
    keys = nc.TILE_SHARED
    nodes = _nodes(keys)
    assert nodes[0][0] is nodes[1][0] is nodes[2][0]
    ctx = gp.Context(300, 0, 0, profile=True)
    got = _call(gp, ctx, keys, True, "tile counts")
    assert not any(np.array_equal(got[i]["dF"], got[j]["dF"]) for i, j in ((0, 1), (0, 2), (1, 2)))
    _same_bits(gp.nodesLogpdfGrad(nodes[:1], ctx)[0], got[0])


# ---- 5. chunks and streams in node mode ---------------------------------------------------------------------------------------------

TUNINGS = (dict(max_batch=2), dict(n_streams=1), dict(n_streams=3), dict(max_batch=2, n_streams=3))


def _chunked(gp, keys, tunings):
    """The call under the default tuning (checked against the reference) and under every tuning of `tunings`, twice each: the same
    bits, and the tuned call against the reference in its own right.  That max_batch = 2 gives ceil(count / 2) chunks is established from the profile: a chunk's per-column factorisation
    issues the same launches whatever the chunk holds (the matrices of a chunk are one batched launch), so classes 0 and 1 record
    ceil(count / 2) times the launches of the default tuning's single chunk — and exactly the default's without max_batch."""
    n, count = keys[0][1], len(keys)
    nodes = _nodes(keys)
    ctx = gp.Context(n, 0, 0, profile=True)
    ref = _call(gp, ctx, keys, True, "chunks")
    _, tr0 = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    assert tr0[4] == 0 and tr0[0] + tr0[1] > 0, tr0
    for tuning in tunings:
        tuned = gp.Context(n, 0, 0, profile=True)
        tuned.set_tuning(**tuning)
        chunks = -(-count // tuning["max_batch"]) if "max_batch" in tuning else 1
        for rep in range(2):
            got, tr = _traced(tuned, lambda: gp.nodesLogpdfGrad(nodes, tuned))
            assert tr == {0: chunks * tr0[0], 1: chunks * tr0[1], 4: 0}, (tuning, rep, tr, tr0)
            for a, b in zip(got, ref):
                _same_bits(a, b)
            assert not tuned.last_info(count).any()
        _check(keys, got, "chunks, tiled")
    return ref


def test_chunks_and_streams_in_node_mode(gp):
    """n = 200, five nodes of widths (3, 8, 0, 16, 1) with different targets: chunks of 2, 2 and 1 nodes read their targets,
    lengthscales, scales and failure codes at s0 = 2 and 4 (GradArgs::y_sstride = n in node mode)"""
    _chunked(gp, nc.CHUNK_KEYS, TUNINGS)


def test_chunks_on_a_shared_feature_block(gp):
    """three nodes on ONE feature block in chunks of 2 and 1: the block is not advanced with s0, the targets are"""
    nodes = _nodes(nc.CHUNK_SHARED)
    assert nodes[0][0] is nodes[1][0] is nodes[2][0]
    _chunked(gp, nc.CHUNK_SHARED, (dict(max_batch=2),))


# ---- 6. many nodes ------------------------------------------------------------------------------------------------------------------

def _repeats_are_identical(got, distinct):
    for i, g in enumerate(got):
        if i >= distinct:
            _same_bits(g, got[i % distinct])


def test_260_nodes_on_the_task_launch(gp):
    """260 nodes at n = 129 cycling over five nodes of widths (0, 1, 3, 8, 16) — and a 261st of 32 columns.  The 260 alone fit the
    single launch (9 blocks hold 27 columns, and 260 <= 4096 nodes), asserted here; they would never reach the task launch.  The
    32-wide node sends the whole call tiled, and its one chunk of 261 >= 256 matrices takes the persistent task launch under a
    full node gradient.  Every repeat of a node has the bits of its first occurrence, and so have the five nodes called beside
    the wide one alone (six matrices: the per-column schedule)."""
    keys = nc.MANY_129
    wide = nc.limit_key(129, 32)
    distinct = _nodes(keys)
    nodes = [distinct[i % 5] for i in range(260)]
    ctx = gp.Context(129, 0, 0, profile=True)
    single, tr = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    assert not _tiled(tr), tr
    _check(keys, single[:5], "many nodes, single launch")
    _repeats_are_identical(single, 5)
    nodes.append(nc.make(wide))
    got, tr = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    assert ctx.profile_get(4)[0] > 0 and tr[4] > 0, tr
    assert not ctx.last_info(261).any()
    _check(keys + [wide], got[:5] + got[260:], "many nodes, task launch")
    _repeats_are_identical(got[:260], 5)
    _logpdf_is_nodes_logpdf(gp, ctx, [keys[i % 5] for i in range(260)] + [wide], nodes, got, False)
    few, tr = _traced(ctx, lambda: gp.nodesLogpdfGrad(distinct + nodes[260:], ctx))
    assert tr[4] == 0 and tr[0] + tr[1] > 0, tr
    for a, b in zip(few, got[:5] + got[260:]):
        _same_bits(a, b)


def test_4097_nodes_on_one_tile(gp):
    """4097 nodes at n = 5 cycling over eight nodes of widths 0 .. 3: more than 4096 nodes send the call to the tiled path, the
    only way to one tile per side in node mode (read from gpslc_nodes_logpdf_grad: `count > 4096`; one tile leaves no trace in
    the profile).  Printed, not asserted: whether the bits are the single launch's."""
    keys = nc.MANY_5
    distinct = _nodes(keys)
    nodes = [distinct[i % 8] for i in range(4097)]
    ctx = gp.Context(5, 0, 0, profile=True)
    got = gp.nodesLogpdfGrad(nodes, ctx)
    assert not ctx.last_info(4097).any()
    _check(keys, got[:8], "many nodes, one tile")
    _repeats_are_identical(got, 8)
    assert np.array_equal(gp.nodesLogpdf(nodes, ctx), [g["logpdf"] for g in got])
    single = gp.nodesLogpdfGrad(distinct, ctx)
    _check(keys, single, "many nodes, the same on the single launch")
    same = all(np.array_equal(np.asarray(a[o]), np.asarray(b[o])) for a, b in zip(single, got) for o in OUT + ("logpdf",))
    print("4097 nodes at n = 5: bit-identical to the single launch:", same)
