"""gpslc_nodes_logpdf_grad on an MI355X against the long-double restatement (tests/node_grad_restatement.py).

Bound per element: tol * scale, tol = max(1e-10, 1e-14 cond(A)), the scale being the same sum with |alpha_r||alpha_c| +
sqrt(c_r c_c) for Q_rc and |D| for D — §21's bound.  tests/test_node_grad.py shows on the CPU that these inputs see an unmasked
padding (dnoise, dscale) and a missing transposed-block contribution (dF) by more than 1e6 bounds, on the single-launch kernel's
16 x 16 blocks and on the 128 x 128 tiles.  Which path ran is asserted from the profile counters where the tiled factorisation
leaves a trace (n > 128), as tests/test_gpu_path_limits.py does.

Measured on one MI355X, worst fraction of the bound: 2.2e-5 on the single launch, 9.7e-5 tiled (both dtarget; dF <= 1.1e-5), and with
features at offset 1e6 0.25 (single launch, n = 48) and 0.68 (tiled, n = 200).  The :Y node through this call and through
gpslc_y_logpdf_grad agree within the bounds and not to the bit, at n = 150 and at n = 200 (DESIGN.md §23 says why)."""
import ctypes as C

import numpy as np
import pytest

import cases
import grad_restatement as gr
import node_grad_restatement as ng

pytestmark = pytest.mark.gpu

FEATURES = (0, 1, 3, 8, 16)
OUT = ng.OUTPUTS
WORST = {}


def _traced(ctx, fn):
    ctx.profile_reset()
    out = fn()
    return out, sum(ctx.profile_get(k)[0] for k in (0, 1, 4)) > 0


def _nodes(keys):
    return [ng.random_node(*k) for k in keys]


def _check(keys, got, what):
    """every node's outputs inside its bound; the shift identity; returns the worst fraction of the bound"""
    worst = 0.0
    for i, (k, g) in enumerate(zip(keys, got)):
        ref, sc, tol, cond = ng.expected(k)
        err = ng.errors(g, ref, sc)
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


def _mixed_keys(n, count, seed):
    return [(n, 8, seed)] if count == 1 else [(n, FEATURES[i % len(FEATURES)], seed + i) for i in range(count)]


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("n", [3, 16, 17, 48, 150])
def test_single_launch(gp, n, count):
    """feature counts 0, 1, 3, 8, 16 mixed in one call; five nodes exceed the descriptors that travel in the kernel arguments"""
    keys = _mixed_keys(n, count, 10 * n)
    nodes = _nodes(keys)
    ctx = gp.Context(n, 0, 0, profile=True)
    got, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    if n > 128:
        assert not tiled
    _check(keys, got, "single launch")
    lp = gp.nodesLogpdf(nodes, ctx)
    assert np.array_equal(lp, [g["logpdf"] for g in got])
    again = gp.nodesLogpdfGrad(nodes, ctx)
    for a, b in zip(got, again):
        _same_bits(a, b)
    assert not ctx.last_info(len(nodes)).any()


def test_the_documented_limit(gp):
    """nF = 8: n = 160 is the last size of the single launch, n = 161 runs tiled; and the same node at n = 160 through both
    paths (a wider node in the call sends it tiled) agrees within the sum of the two bounds"""
    key = (160, 8, 3)
    wide = (160, 32, 4)
    ctx = gp.Context(160, 0, 0, profile=True)
    small, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(_nodes([key]), ctx))
    assert not tiled
    big, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(_nodes([key, wide]), ctx))
    assert tiled
    _check([key], small, "limit, single launch")
    _check([key, wide], big, "limit, tiled")
    ref, sc, tol, _ = ng.expected(key)
    for o in OUT:
        assert np.all(np.abs(np.asarray(small[0][o]) - np.asarray(big[0][o])) <= 2 * tol * np.asarray(sc[o], dtype=np.float64)), o
    ctx1 = gp.Context(161, 0, 0, profile=True)
    got, tiled = _traced(ctx1, lambda: gp.nodesLogpdfGrad(_nodes([(161, 8, 5)]), ctx1))
    assert tiled
    _check([(161, 8, 5)], got, "limit + 1, tiled")


@pytest.mark.parametrize("n,nFs", [(129, (32, 0, 1, 3, 8, 16)), (200, (3, 8, 0))])
def test_tiled_path(gp, n, nFs):
    """two tiles with one live row (n = 129: the 32-column node does not fit the single launch, so the whole call runs tiled) and
    n = 200, on a context without set_data"""
    keys = [(n, nF, 20 * n + i) for i, nF in enumerate(nFs)]
    ctx = gp.Context(n, 0, 0, profile=True)
    got, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(_nodes(keys), ctx))
    assert tiled
    _check(keys, got, "tiled")
    assert not ctx.last_info(len(keys)).any()


def test_tiled_logpdf_is_nodes_logpdf(gp):
    """513 nodes at n = 200 send gpslc_nodes_logpdf to the tiled path too: the same bits"""
    n = 200
    nodes = _nodes([(n, 1, 1000 + i) for i in range(513)])
    ctx = gp.Context(n, 0, 0, profile=True)
    got, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx, want=("dnoise", "logpdf")))
    lp, tiled_lp = _traced(ctx, lambda: gp.nodesLogpdf(nodes, ctx))
    assert tiled and tiled_lp
    assert np.array_equal(lp, [g["logpdf"] for g in got])


def test_tiled_shared_block_and_widest_node(gp):
    """n = 200: three nodes on ONE feature block (the X nodes' F = U) get one gradient block each; a node alone and the same node
    beside a wider one have identical bits; so has a node at another position of the call"""
    n = 200
    shared = [(n, 2, 31, 30), (n, 2, 32, 30), (n, 2, 30)]
    nodes = _nodes(shared)
    assert nodes[0][0] is nodes[1][0] is nodes[2][0]
    ctx = gp.Context(n, 0, 0, profile=True)
    got, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    assert tiled
    _check(shared, got, "tiled")
    alone = gp.nodesLogpdfGrad(nodes[:1], ctx)[0]
    _same_bits(alone, got[0])
    mixed_keys = [(n, 16, 33), (n, 0, 34), shared[0]]
    mixed = gp.nodesLogpdfGrad(_nodes(mixed_keys), ctx)
    _check(mixed_keys, mixed, "tiled")
    _same_bits(alone, mixed[2])


@pytest.mark.parametrize("n", [48, 150])
def test_position_and_subset_on_the_single_launch(gp, n):
    keys = [(n, 3, 40 * n, 40 * n + 9), (n, 3, 40 * n + 1, 40 * n + 9), (n, 8, 40 * n + 2), (n, 0, 40 * n + 3), (n, 16, 40 * n + 4)]
    nodes = _nodes(keys)
    assert nodes[0][0] is nodes[1][0]             # two nodes on one feature block, one pointer
    ctx = gp.Context(n, 0, 0, profile=True)
    full, tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad(nodes, ctx))
    assert not tiled
    _check(keys, full, "single launch")
    for i in (0, 3, 4):       # the node alone (its descriptor in the kernel arguments) against position i (4: read from memory)
        _same_bits(gp.nodesLogpdfGrad(nodes[i:i + 1], ctx)[0], full[i])
    rev = gp.nodesLogpdfGrad(nodes[::-1], ctx)
    for i in range(5):
        _same_bits(rev[4 - i], full[i])
    for want in (("dF",), ("dls", "dnoise"), ("dscale", "dtarget", "logpdf"), ("dtarget",)):
        part = gp.nodesLogpdfGrad(nodes, ctx, want=want)
        for a, b in zip(part, full):
            _same_bits(a, b, want)
            assert all(a[o] is None for o in OUT + ("logpdf",) if o not in want)


def test_subset_on_the_tiled_path(gp):
    n = 200
    keys = [(n, 3, 51), (n, 8, 52)]
    ctx = gp.Context(n, 0, 0)
    full = gp.nodesLogpdfGrad(_nodes(keys), ctx)
    for want in (("dF",), ("dls",), ("dscale", "dnoise", "dtarget"), ("dtarget", "logpdf")):
        part = gp.nodesLogpdfGrad(_nodes(keys), ctx, want=want)
        for a, b in zip(part, full):
            _same_bits(a, b, want)
    again = gp.nodesLogpdfGrad(_nodes(keys), ctx)
    for a, b in zip(again, full):
        _same_bits(a, b)


@pytest.mark.parametrize("n", [150, 200])
def test_y_node_against_y_logpdf_grad(gp, n):
    """the :Y node (F = [U | X | T]) through this call against gpslc_y_logpdf_grad: within the sum of the two bounds — at n = 150
    one side is the single launch; at n = 200 both are tiled, but the node call carries T as a feature column where the outcome
    call multiplies a separate treatment factor into K, so the two factorise matrices that differ in their last bits"""
    c = cases.make_case(n, "UX", False, S=1, seed=60 + n)
    g = cases.gpslc_object(gp, c)
    st, yg = g.ctx().y_logpdf_grad(1, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise)
    assert st == 0
    W, ls, nU, nX, ys, yn, Y = gr.inputs(c, 0)
    node = (np.asfortranarray(W), ls, ys, yn, Y)
    ctx = gp.Context(n, 0, 0, profile=True)
    (ng_out,), tiled = _traced(ctx, lambda: gp.nodesLogpdfGrad([node], ctx))
    assert tiled == (n > 176)
    ref = gr.expected(c)[0]
    tol, sc = ref["tol"], ref["scales"]
    pairs = [(ng_out["dF"][:, :nU], yg["dU"][:, :, 0], sc["dU"]), (ng_out["dls"][:nU], yg["duyLS"][:, 0], sc["duyLS"]),
             (ng_out["dls"][nU:nU + nX], yg["dxyLS"][:, 0], sc["dxyLS"]), (ng_out["dls"][-1], yg["dtyLS"][0], sc["dtyLS"]),
             (ng_out["dscale"], yg["dyScale"][0], sc["dyScale"]), (ng_out["dnoise"], yg["dyNoise"][0], sc["dyNoise"]),
             (ng_out["dtarget"], yg["dY"][:, 0], sc["dY"])]
    bits = all(np.array_equal(a, b) for a, b, _ in pairs)
    print("n", n, "bit-identical to gpslc_y_logpdf_grad:", bits)
    for a, b, s in pairs:
        assert np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 2 * tol * np.asarray(s, dtype=np.float64))
    gn, sn = ng.gradient(node, np.longdouble)
    err = ng.errors(ng_out, gn, sn)
    assert max(err.values()) <= tol, err


def _singular(n, nF=3, seed=70):
    """duplicate rows, noise = 0, scale = 1: pivot 2 is exactly 0"""
    F, ls, _, _, y = ng.random_node(n, nF, seed)
    F = F.copy(order="F")
    F[1] = F[0]
    return (F, ls, 1.0, 0.0, y)


@pytest.mark.parametrize("n", [48, 200])
def test_a_singular_node_between_good_ones(gp, n):
    keys = [(n, 3, 71), (n, 8, 72)]
    good = _nodes(keys)
    nodes = [good[0], _singular(n), good[1]]
    ctx = gp.Context(n, 0, 0)
    st, out = ctx.nodes_logpdf_grad(nodes)
    assert st == 2
    assert list(ctx.last_info(3)) == [0, 2, 0]
    dF, dls = out["dF"], out["dls"]
    assert np.isnan(dF[3 * n:6 * n]).all() and np.isnan(dls[3:6]).all()
    assert np.isnan(out["dscale"][1]) and np.isnan(out["dnoise"][1]) and np.isnan(out["dtarget"][:, 1]).all()
    got = [dict(dF=dF[:3 * n].reshape((n, 3), order="F"), dls=dls[:3], dscale=out["dscale"][0], dnoise=out["dnoise"][0],
                dtarget=out["dtarget"][:, 0]),
           dict(dF=dF[6 * n:].reshape((n, 8), order="F"), dls=dls[6:], dscale=out["dscale"][2], dnoise=out["dnoise"][2],
                dtarget=out["dtarget"][:, 2])]
    _check(keys, got, "beside a breakdown")
    with pytest.raises(gp.PosDefException) as ei:
        gp.nodesLogpdfGrad(nodes, ctx)
    assert ei.value.info == 2


def test_argument_errors(gp):
    n = 24
    nodes = _nodes([(n, 3, 80), (n, 0, 81)])
    ctx = gp.Context(n, 0, 0)
    assert ctx.nodes_logpdf_grad(nodes, want=())[0] == -4
    assert ctx.nodes_logpdf_grad(nodes, want=("logpdf",))[0] == -4          # logpdf alone is gpslc_nodes_logpdf's call
    assert b"NULL" in ctx.lib.gpslc_last_error(ctx.h)
    buf = np.zeros(4 * n)
    p = buf.ctypes.data
    assert ctx.lib.gpslc_nodes_logpdf_grad(ctx.h, -1, None, p, None, None, None, None, None) == -2
    assert ctx.lib.gpslc_nodes_logpdf_grad(ctx.h, 2, None, p, None, None, None, None, None) == -3
    arr, _keep = gp.api._marshal_nodes(nodes, ctx)
    arr[0].nF = 33
    assert ctx.lib.gpslc_nodes_logpdf_grad(ctx.h, 2, C.cast(arr, C.c_void_p), p, None, None, None, None, None) == -3
    st, out = ctx.nodes_logpdf_grad([])                                         # an empty call
    assert st == 0 and out["dtarget"].shape == (n, 0) and out["dF"].shape == (0,)
    f32 = gp.Context(n, 0, 0, fp32_kernel=True)
    assert f32.nodes_logpdf_grad(nodes)[0] == -1007                             # GPSLC_ERR_UNSUPPORTED
    assert b"fp64" in f32.lib.gpslc_last_error(f32.h)
    st, out = ctx.nodes_logpdf_grad(nodes)                                      # and the good call still runs
    assert st == 0 and out["dF"].shape == (3 * n,) and out["dls"].shape == (3,)


@pytest.mark.parametrize("n", [48, 200])
def test_features_off_the_unit_scale(gp, n):
    """features at offset 1e6 with spread 1: D comes from the raw features, so dF and dls keep their digits"""
    key = (n, 3, 90, None, 1e6)
    ctx = gp.Context(n, 0, 0)
    _check([key], gp.nodesLogpdfGrad(_nodes([key]), ctx), "off the unit scale")


@pytest.mark.parametrize("binary,nU,with_x", [(False, 2, True), (True, 2, True), (False, 2, False)])
def test_grad_xty_on_a_chain(gp, binary, nU, with_x):
    """`_RealTChain.grad_xty` at n = 40 against the node-by-node restatement put together with this test's own index mapping;
    the bound of a sum is the sum of the nodes' bounds"""
    from causalgpslc_jl_amd import inference as inf
    n, nX = 40, 3 if with_x else 0
    rng = np.random.default_rng(95)
    X = rng.standard_normal((n, nX)) if nX else None
    T = (rng.random(n) < 0.5) if binary else rng.standard_normal(n)
    Y = rng.standard_normal(n)
    SigmaU = inf.generateSigmaU([5] * (n // 5), eps=1e-6)
    pp = gp.getPriorParameters()
    pp["SigmaU"] = SigmaU
    ch = inf._RealTChain(pp, SigmaU, X, T, Y, nU, np.random.Generator(np.random.Philox(7)), binary=binary)
    g = ch.grad_xty()
    nodes, nx, has_t = ch._xty_nodes(ch.v, None)
    assert nx == nX and has_t and len(nodes) == nX + 2
    ref = []
    for nd in nodes:
        gl, sl = ng.gradient(nd, np.longdouble)
        ref.append((gl, sl, ng.node_tolerance(nd)[0]))

    def close(got, want, bound, what):
        assert np.all(np.abs(np.asarray(got, dtype=np.longdouble) - want) <= np.asarray(bound, dtype=np.longdouble)), what

    # dUm: every X node's whole block, the first nU columns of the T and Y nodes
    want = sum(r[0]["dF"][:, :nU] for r in ref)
    bound = sum(r[2] * r[1]["dF"][:, :nU] for r in ref)
    close(g["dUm"], want, bound, "dUm")
    for u in range(nU):          # traced vector u, individual i is element u + nU i of the flattened model matrix
        for i in range(n):
            p = u + nU * i
            close(g["dU"][u][i], want[p % n, p // n], bound[p % n, p // n], ("dU", u, i))
    for k in range(nX):          # X node k reads row k of the (nX, nU) model matrix: element k + nX c is uxLS[p % nU][p // nU]
        gl, sl, tol = ref[k]
        for c in range(nU):
            p = k + nX * c
            close(g["uxLS"][p % nU, p // nU], gl["dls"][c], tol * sl["dls"][c], ("uxLS", k, c))
        close(g["xScale"][k], gl["dscale"], tol * sl["dscale"], "xScale")
        close(g["xNoise"][k], gl["dnoise"], tol * sl["dnoise"], "xNoise")
    gl, sl, tol = ref[nX]
    close(g["utLS"], gl["dls"][:nU], tol * sl["dls"][:nU], "utLS")
    close(g["tScale"], gl["dscale"], tol * sl["dscale"], "tScale")
    close(g["tNoise"], gl["dnoise"], tol * sl["dnoise"], "tNoise")
    if nX:
        close(g["xtLS"], gl["dls"][nU:], tol * sl["dls"][nU:], "xtLS")
    if binary:
        close(g["dlogitT"], gl["dtarget"], tol * sl["dtarget"], "dlogitT")
    else:
        assert "dlogitT" not in g
    gl, sl, tol = ref[-1]
    close(g["uyLS"], gl["dls"][:nU], tol * sl["dls"][:nU], "uyLS")
    if nX:
        close(g["xyLS"], gl["dls"][nU:nU + nX], tol * sl["dls"][nU:nU + nX], "xyLS")
    close(g["tyLS"], gl["dls"][-1], tol * sl["dls"][-1], "tyLS")
    close(g["yScale"], gl["dscale"], tol * sl["dscale"], "yScale")
    close(g["yNoise"], gl["dnoise"], tol * sl["dnoise"], "yNoise")
