"""Node and MVN scores on both sides of the switch between the single-workgroup kernels and the batched tiled path
(fast_path_ok, csrc/api_score.hip): a call takes the single-workgroup kernels (k_small.hip) for n <= 640 and at most 4096 nodes
(the matrix fits LDS) or 512 (the left-looking kernel, n up to 640), the batched tiled factorisation otherwise — and that
path runs the persistent task launch (potrf_tasks_kernel) for chunks of >= 256 matrices.  The MH chain crosses these
counts (score_xty_many and the batched sweep of inference.py score len(Us) x (nX + 2) nodes per call), so every call here
is checked against the batched fp64 host reference (tests/batched_reference.py), the two sides of each limit against each
other, and which path ran is asserted from the profile counters: the tiled factorisation records launches in kernel
classes 0, 1 (per-column schedule) or 4 (task launch); the single-workgroup kernels record none.  Every size has at least
two tiles per side (n >= 129), so that the tiled schedule leaves a trace.

The MVN node (gpslc_mvn_logpdf / gpslc_mvn_draw) caches the handed-over covariance; cov = None must mean the latest one
whichever path either call took (test_mvn_cache_follows_the_latest_covariance_across_the_limit)."""
import ctypes as C

import numpy as np
import pytest

import batched_reference as br
import cases
import gpslc_oracle as orc

pytestmark = pytest.mark.gpu

TILE = 128
NODE_RTOL, NODE_ATOL = 1e-10, 1e-9           # the suite's node tolerances
SIDES_RTOL = 1e-11                           # the same node on both sides of a limit
FEATURES = (0, 1, 3, 8, 16)


def _ctx(gp, n, nX=0, nU=0):
    assert n > TILE, "a tiled factorisation of one tile per side would leave no trace in the profile"
    return gp.Context(n, nX, nU, profile=True)


def _traced(ctx, fn):
    """fn() and the launches of the tiled factorisation it recorded: {class: launches} for classes 0, 1, 4"""
    ctx.profile_reset()
    out = fn()
    return out, {k: ctx.profile_get(k)[0] for k in (0, 1, 4)}


def _tiled(tr):
    return sum(tr.values()) > 0


def _nodes(n, count, seed, nFs=FEATURES):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        nF = nFs[i % len(nFs)]
        F = None if nF == 0 else rng.standard_normal((n, nF))
        ls = None if nF == 0 else rng.uniform(0.8, 2.5, nF)
        out.append((F, ls, rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.5), rng.standard_normal(n)))
    return out


def _close(got, ref, rtol=NODE_RTOL, atol=NODE_ATOL):
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref) - (atol + rtol * np.abs(ref))
    assert np.all(err <= 0), (int(np.argmax(err)), float(np.max(err)))


def _same_sides(a, b, rtol=SIDES_RTOL):
    assert np.all(np.abs(a - b) <= rtol * np.abs(b)), float(np.max(np.abs(a - b) / np.abs(b)))


def _draws_close(got, ref, rtol=1e-9, atol_rel=1e-10):
    for i in range(ref.shape[1]):
        assert np.allclose(got[:, i], ref[:, i], rtol=rtol, atol=atol_rel * np.abs(ref[:, i]).max()), \
            (i, float(np.abs(got[:, i] - ref[:, i]).max()))


LIMITS = [(150, 4096), (300, 512), (640, 512)]   # (n, the last count the single-workgroup kernels take)


@pytest.mark.parametrize("n,lim", LIMITS)
def test_nodes_logpdf_at_the_count_limit(gp, n, lim):
    """gpslc_nodes_logpdf with feature counts 0, 1, 3, 8, 16 mixed in one call: lim nodes on the single-workgroup kernels, lim + 1
    (the same nodes and one more) on the batched tiled path."""
    nodes = _nodes(n, lim + 1, seed=n + lim)
    ref = br.node_scores(nodes)["logpdf"]
    ctx = _ctx(gp, n)
    small, tr_s = _traced(ctx, lambda: gp.nodesLogpdf(nodes[:lim], ctx))
    big, tr_b = _traced(ctx, lambda: gp.nodesLogpdf(nodes, ctx))
    assert not _tiled(tr_s) and _tiled(tr_b), (tr_s, tr_b)
    _close(small, ref[:lim])
    _close(big, ref)
    _same_sides(big[:lim], small)
    assert not ctx.last_info(lim + 1).any()


@pytest.mark.parametrize("n,lim", LIMITS)
def test_gp_logpdf_at_the_count_limit(gp, n, lim):
    """gpslc_gp_logpdf with per-set feature blocks (nF = 3) and per-set targets, S = lim and lim + 1"""
    rng = np.random.default_rng(7 * n + lim)
    S, nF = lim + 1, 3
    F = rng.standard_normal((n, nF, S))
    ls = rng.uniform(0.8, 2.5, (nF, S))
    sc, nz = rng.uniform(0.5, 2.0, S), rng.uniform(0.2, 1.5, S)
    tg = rng.standard_normal((n, S))
    ref = br.node_scores([(F[:, :, s], ls[:, s], sc[s], nz[s], tg[:, s]) for s in range(S)])["logpdf"]
    ctx = _ctx(gp, n)
    small, tr_s = _traced(ctx, lambda: gp.gpLogpdf(F[:, :, :lim], ls[:, :lim], sc[:lim], nz[:lim], tg[:, :lim], ctx=ctx))
    big, tr_b = _traced(ctx, lambda: gp.gpLogpdf(F, ls, sc, nz, tg, ctx=ctx))
    assert not _tiled(tr_s) and _tiled(tr_b), (tr_s, tr_b)
    _close(small, ref[:lim])
    _close(big, ref)
    _same_sides(big[:lim], small)


def _sub(c, S):
    """the first S posterior samples of a case"""
    d = dict(c)
    d["S"] = S
    for k in ("U", "uyLS", "xyLS", "tyLS", "yNoise", "yScale"):
        if d[k] is not None:
            d[k] = np.asfortranarray(d[k][..., :S])
    return d


@pytest.mark.parametrize("n,lim", LIMITS)
def test_y_logpdf_at_the_count_limit(gp, n, lim):
    """gpslc_y_logpdf (nF_max = nU + nX + 1 = 6 with the treatment column) for S = lim and lim + 1 posterior samples"""
    c = cases.make_case(n, "UX", False, S=lim + 1, seed=n + lim)
    assert np.min(c["yNoise"]) >= 0.2
    ref = br.structured_batch(c["X"], c["T"], c["Y"], c, range(lim + 1), [0.0])["logpdf"]
    ctx = _ctx(gp, n, c["X"].shape[1], c["U"].shape[1])
    ctx.set_data(c["X"], c["T"], c["Y"])
    g_s = cases.gpslc_object(gp, _sub(c, lim), _ctx=ctx)
    g_b = cases.gpslc_object(gp, c, _ctx=ctx)
    small, tr_s = _traced(ctx, lambda: gp.yLogpdf(g_s))
    big, tr_b = _traced(ctx, lambda: gp.yLogpdf(g_b))
    assert not _tiled(tr_s) and _tiled(tr_b), (tr_s, tr_b)
    _close(small, ref[:lim])
    _close(big, ref)
    _same_sides(big[:lim], small)


def test_tiled_node_schedules_are_bit_identical(gp):
    """n = 300 (3 tiles), 513 nodes: the default schedule runs the persistent task launch; the per-column schedule
    (set_task_schedule(2, 0)) gives the same scores and draws bit for bit, and so does a call chunked (max_batch = 300) into a
    task-launch chunk of 300 and a per-column chunk of 213."""
    n, count = 300, 513
    nodes = _nodes(n, count, seed=17)
    ref = br.node_scores(nodes)
    runs = []
    for mode in ("tasks", "columns", "mixed"):
        ctx = _ctx(gp, n)
        if mode == "columns":
            ctx.set_task_schedule(2, 0)
        if mode == "mixed":
            ctx.set_tuning(max_batch=300)
        lp, tr = _traced(ctx, lambda: gp.nodesLogpdf(nodes, ctx))
        dr, tr_d = _traced(ctx, lambda: gp.nodesDraw(nodes, ctx))
        if mode == "tasks":
            assert tr[4] > 0 and tr_d[4] > 0, (tr, tr_d)
        elif mode == "columns":
            assert tr[4] == 0 and tr[0] + tr[1] > 0, tr
        else:
            assert tr[4] == 1 and tr[0] + tr[1] > 0, tr        # one persistent chunk, one per-column chunk
        _close(lp, ref["logpdf"])
        _draws_close(dr, ref["draw"])
        runs.append((lp, dr))
    for lp, dr in runs[1:]:
        assert np.array_equal(lp, runs[0][0])
        assert np.array_equal(dr, runs[0][1])


def test_tiled_gp_logpdf_shared_features_and_target(gp):
    """gpslc_gp_logpdf past the count limit with one feature block for all sets (f_shared = 1), one target for all sets
    (t_shared = 1), and both; the count-512 call on the single-workgroup kernels agrees on the shared sets."""
    n, S, nF = 300, 513, 4
    rng = np.random.default_rng(23)
    F = rng.standard_normal((n, nF))
    Fs = rng.standard_normal((n, nF, S))
    ls = rng.uniform(0.8, 2.5, (nF, S))
    sc, nz = rng.uniform(0.5, 2.0, S), rng.uniform(0.2, 1.5, S)
    t1 = rng.standard_normal(n)
    ts = rng.standard_normal((n, S))
    ctx = _ctx(gp, n)
    for FF, tt in ((F, ts), (Fs, t1), (F, t1)):
        ref = br.node_scores([(FF if FF.ndim == 2 else FF[:, :, s], ls[:, s], sc[s], nz[s], tt if tt.ndim == 1 else tt[:, s])
                              for s in range(S)])["logpdf"]
        big, tr = _traced(ctx, lambda: gp.gpLogpdf(FF, ls, sc, nz, tt, ctx=ctx))
        small, tr_s = _traced(ctx, lambda: gp.gpLogpdf(FF if FF.ndim == 2 else FF[:, :, :512], ls[:, :512], sc[:512], nz[:512],
                                                        tt if tt.ndim == 1 else tt[:, :512], ctx=ctx))
        assert tr[4] > 0 and not _tiled(tr_s), (tr, tr_s)
        _close(big, ref)
        _same_sides(big[:512], small)


def test_tiled_nodes_with_one_shared_feature_block_and_32_features(gp):
    """gpslc_nodes_logpdf past the count limit when every node hands over the same F (the same_f branch of nodes_general: F
    staged once), and with nF = 32 (the widest block) mixed with narrower nodes"""
    n, count = 300, 513
    rng = np.random.default_rng(29)
    F = rng.standard_normal((n, 5))
    nodes = [(F, rng.uniform(0.8, 2.5, 5), rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.5), rng.standard_normal(n))
             for _ in range(count)]
    ctx = _ctx(gp, n)
    out, tr = _traced(ctx, lambda: gp.nodesLogpdf(nodes, ctx))
    assert tr[4] > 0, tr
    _close(out, br.node_scores(nodes)["logpdf"])
    _same_sides(out[:512], gp.nodesLogpdf(nodes[:512], ctx))
    wide = _nodes(n, count, seed=31, nFs=(32, 0, 7, 32))
    out, tr = _traced(ctx, lambda: gp.nodesLogpdf(wide, ctx))
    assert tr[4] > 0, tr
    _close(out, br.node_scores(wide)["logpdf"])
    small, tr_s = _traced(ctx, lambda: gp.nodesLogpdf(wide[:512], ctx))
    assert not _tiled(tr_s), tr_s
    _same_sides(out[:512], small)


def test_failing_nodes_at_queue_and_chunk_edges(gp):
    """513 nodes on the task launch, four of them not positive definite (first, last, and either side of 256): exactly those
    report their pivot (LAPACK's, as the reference's) and get fail_value; every other score is bit-identical to the call
    without them."""
    n, count = 300, 513
    nodes = _nodes(n, count, seed=37)
    bad = [0, 255, 256, 512]
    broken = list(nodes)
    for i in bad:
        F, ls, sc, _, tg = nodes[i]
        broken[i] = (F, ls, sc, -sc - 1.0, tg)                 # first diagonal entry sc + noise = -1
    ref = br.node_scores(broken)
    assert (np.flatnonzero(ref["info"]) == bad).all()
    ctx = _ctx(gp, n)
    good = gp.nodesLogpdf(nodes, ctx)
    out, tr = _traced(ctx, lambda: gp.nodesLogpdf(broken, ctx, fail_value=-np.inf))
    assert tr[4] > 0, tr
    info = ctx.last_info(count)
    assert np.array_equal(np.flatnonzero(info), bad), np.flatnonzero(info)
    assert np.array_equal(info, ref["info"]), info[bad]
    assert np.array_equal(np.flatnonzero(out == -np.inf), bad)
    keep = np.setdiff1d(np.arange(count), bad)
    assert np.array_equal(out[keep], good[keep])
    with pytest.raises(gp.PosDefException) as ei:
        gp.nodesLogpdf(broken, ctx)
    assert ei.value.info == 1


def test_nodes_draw_past_the_count_limit(gp):
    """gpslc_nodes_draw for 513 nodes (task launch + the predictive-draw kernel) against chol(K) z, and against the count-512
    call (single-workgroup draw mode) on the shared nodes"""
    n, count = 300, 513
    nodes = _nodes(n, count, seed=41)
    ref = br.node_scores(nodes)["draw"]
    ctx = _ctx(gp, n)
    big, tr = _traced(ctx, lambda: gp.nodesDraw(nodes, ctx))
    small, tr_s = _traced(ctx, lambda: gp.nodesDraw(nodes[:512], ctx))
    assert tr[4] > 0 and not _tiled(tr_s), (tr, tr_s)
    _draws_close(big, ref)
    _draws_close(small, ref[:, :512])
    _draws_close(big[:, :512], small, rtol=1e-10, atol_rel=1e-11)


# ---- the MVN node ------------------------------------------------------------------------------------------------------

def _sigma(n, seed):
    """generate_sigma_u with objects of 5 and a 1e-3 jitter (cond ~ 5e3), rows and columns shuffled"""
    sizes = [5] * (n // 5) + ([n % 5] if n % 5 else [])
    Sig = orc.generate_sigma_u(sizes, 1e-3, 1.0)
    p = np.random.default_rng(seed).permutation(n)
    return np.ascontiguousarray(Sig[np.ix_(p, p)])


def _gram(n, seed):
    G = np.random.default_rng(seed).standard_normal((n, n // 2))
    return G @ G.T / (n // 2) + 0.5 * np.eye(n)


@pytest.mark.parametrize("n,Ss,tiled_from", [(700, (1, 127, 128, 129, 300), 1), (1100, (1, 127, 128, 129, 300), 1),
                                             (300, (512, 513), 513), (150, (4096, 4097), 4097)])
def test_mvn_scores_and_draws_across_the_limits(gp, n, Ss, tiled_from):
    """gpslc_mvn_logpdf / gpslc_mvn_draw with per-vector covscale: several right-hand-side tiles on the tiled path (S > 128),
    the single-workgroup kernels up to the count limit and the tiled path past it; both sides agree."""
    cov = _sigma(n, n)
    rng = np.random.default_rng(n + 1)
    Smax = max(Ss)
    X = rng.standard_normal((n, Smax))
    Z = rng.standard_normal((n, Smax))
    cs = rng.uniform(0.3, 3.0, Smax)
    ref = br.mvn_scores(cov, X, cs)
    refd = br.mvn_scores(cov, Z, cs)["draw"]
    ctx = _ctx(gp, n)
    got = {}
    for i, S in enumerate(Ss):
        lp, tr = _traced(ctx, lambda: gp.mvnLogpdf(cov if i == 0 else None, X[:, :S], cs[:S], ctx=ctx))
        assert _tiled(tr) == (S >= tiled_from), (S, tr)
        dr = gp.mvnDraw(None, Z[:, :S], cs[:S], ctx=ctx)
        _close(lp, ref["logpdf"][:S], rtol=1e-10, atol=0)
        _draws_close(dr, refd[:, :S], rtol=0, atol_rel=1e-9)
        assert not ctx.last_info(S).any()
        got[S] = (lp, dr)
    if tiled_from > 1:
        a, b = Ss
        _same_sides(got[b][0][:a], got[a][0])
        _draws_close(got[b][1][:, :a], got[a][1], rtol=0, atol_rel=1e-11)


def _bad_cov(n, j):
    """positive definite except at pivot j (LAPACK info j + 1), as test_gpu_model_nodes builds it"""
    rng = np.random.default_rng(j)
    d = 1.0 + rng.random(n)
    d[j] = -0.5
    cov = np.diag(d)
    if j > 2:
        v = 0.1 * rng.standard_normal(j)
        cov[:j, :j] += np.outer(v, v)
    return cov


def _raw_mvn(ctx, S, x, draw=False):
    """the C entry point with cov = NULL: (status, outputs)"""
    x = np.asfortranarray(x)
    out = np.zeros((ctx.n, S) if draw else S, order="F")
    fn = ctx.lib.gpslc_mvn_draw if draw else ctx.lib.gpslc_mvn_logpdf
    st = fn(ctx.h, S, None, None, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return st, out


@pytest.mark.parametrize("j", [0, 1, 127, 128, 129, 255, 256, 640, 799])
def test_failing_pivot_on_the_tiled_mvn_path(gp, j):
    """n = 800 (robust tiled factorisation of the cached covariance): PosDefException(j + 1) for the hand-over, and for every
    later cov = None call of either entry point, whose outputs are NaN; last_info holds j + 1 for every vector."""
    n, S = 800, 3
    cov = _bad_cov(n, j)
    rng = np.random.default_rng(800 + j)
    x = rng.standard_normal((n, S))
    ctx = _ctx(gp, n)
    with pytest.raises(gp.PosDefException) as ei:
        gp.mvnLogpdf(cov, x, ctx=ctx)
    assert ei.value.info == j + 1
    assert (ctx.last_info(S) == j + 1).all()
    for fn in (gp.mvnLogpdf, gp.mvnDraw):
        with pytest.raises(gp.PosDefException) as ei:
            fn(None, x, ctx=ctx)
        assert ei.value.info == j + 1
        assert (ctx.last_info(S) == j + 1).all()
    for draw in (False, True):
        st, out = _raw_mvn(ctx, S, x, draw)
        assert st == j + 1 and np.isnan(out).all()


def test_mvn_cache_follows_the_latest_covariance_across_the_limit(gp):
    """n = 300: calls of up to 512 vectors run the single-workgroup kernels on the kept matrix, 513 the tiled factor.  cov = None
    must mean the covariance handed over last — whichever path either hand-over took, for mvnLogpdf and mvnDraw — and must
    work on a path that has not been built yet; a non-positive-definite hand-over fails every later cov = None call."""
    n, few, many = 300, 3, 513
    A, B = _sigma(n, 1), _gram(n, 2)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, many))
    Z = rng.standard_normal((n, many))
    cs = rng.uniform(0.5, 2.0, many)
    refs = {}
    for name, M in (("A", A), ("B", B)):
        refs[name] = (br.mvn_scores(M, X, cs)["logpdf"], br.mvn_scores(M, Z, cs)["draw"])

    def score(ctx, cov, S, want):
        lp, tr = _traced(ctx, lambda: gp.mvnLogpdf(cov, X[:, :S], cs[:S], ctx=ctx))
        assert _tiled(tr) == (S > 512), (S, tr)
        _close(lp, refs[want][0][:S], rtol=1e-10, atol=0)

    def draw(ctx, cov, S, want):
        _draws_close(gp.mvnDraw(cov, Z[:, :S], cs[:S], ctx=ctx), refs[want][1][:, :S], rtol=0, atol_rel=1e-9)

    ctx = _ctx(gp, n)
    # tiled A, then dense B: None on the tiled side must be B
    score(ctx, A, many, "A")
    score(ctx, B, few, "B")
    score(ctx, None, many, "B")
    draw(ctx, None, many, "B")
    draw(ctx, None, few, "B")
    # dense A, then tiled B: None on the dense side must be B
    score(ctx, A, few, "A")
    score(ctx, B, many, "B")
    score(ctx, None, few, "B")
    draw(ctx, None, few, "B")
    score(ctx, None, many, "B")
    # hand-overs through mvnDraw, on either side
    draw(ctx, A, many, "A")
    score(ctx, None, few, "A")
    draw(ctx, B, few, "B")
    score(ctx, None, many, "B")
    draw(ctx, None, many, "B")
    # cov = None on a path never built in this context
    for first, then in ((few, many), (many, few)):
        fresh = _ctx(gp, n)
        score(fresh, A, first, "A")
        score(fresh, None, then, "A")
        draw(fresh, None, then, "A")
    # a non-positive-definite hand-over on either side: every later cov = None call reports its pivot, on both sides
    j = 200
    bad = _bad_cov(n, j)
    for side in (few, many):
        score(ctx, A, many, "A")
        score(ctx, A, few, "A")
        with pytest.raises(gp.PosDefException) as ei:
            gp.mvnLogpdf(bad, X[:, :side], ctx=ctx)
        assert ei.value.info == j + 1
        for S in (few, many):
            for fn, V in ((gp.mvnLogpdf, X), (gp.mvnDraw, Z)):
                with pytest.raises(gp.PosDefException) as ei:
                    fn(None, V[:, :S], cs[:S], ctx=ctx)
                assert ei.value.info == j + 1, (side, S, fn.__name__)
                assert (ctx.last_info(S) == j + 1).all()
    # and a good hand-over afterwards serves both sides again
    score(ctx, B, few, "B")
    score(ctx, None, many, "B")
    draw(ctx, None, many, "B")
