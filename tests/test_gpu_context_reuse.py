"""One context serving calls of changing size: every buffer a gpslc_ctx owns (csrc/dev_mem.h, csrc/host_ctx.h) is made to grow and
is then used again at a smaller size, and the last call of each sequence is compared BIT FOR BIT with the same call on a fresh
context.  Growth has no other observable effect: a buffer that lost its contents' owner, kept a stale size or pointer, or was
freed under a launch shows as different bytes (or as a fault), never as a status.  Every status is GPSLC_OK: the front end raises
on any other.  The shapes are the smallest that reach each buffer:

* the slot arenas and the progress words of the persistent factorisation launch — n = 300 (three tiles per side, so the trailing
  update's visiting order, tri_order, is live), the launch forced for every chunk, predict with S = 8, 64, 8; and under two
  streams with chunks of at most 32 samples, where S = 8, 40, 64, 8 makes the first slot's words grow (8 -> 32 matrices) while
  the second's are allocated (8), then the second's grow (8 -> 32) while the first's do not;
* the cache of task lists (eight shapes, least recently used evicted) — nine (S, back-substitution yes / no) shapes, then the first;
* the call-level scratch — a draws-only predict (the internal MeanITE), S = 4, 16, 4, and the mid-size node kernel's per-node
  columns at n = 300 with 2, 8, 2 nodes;
* the pinned staging of the single-launch node scores — n = 40 with 2, 50, 2 nodes, then the gradient launch on the same context;
* the staging pool's chain and merge — yLogpdf at n = 300, nU = 2 with S = 4, then S = 512 (2.4 MB of U: beyond the first 1 MiB
  block), then S = 4 twice (the merged block, then steady state);
* the MVN cache — n = 300, where both paths run: a covariance handed over on the single-workgroup path, cov = None on the tiled
  path (S > 512: the factor is built from the dense copy), a second covariance, cov = None on each path, against fresh contexts
  given the second covariance directly; and n = 700, where the tiled factor is all there is;
* create / use / destroy, 20 times in one process.

No test here looks at free device memory: the devices are shared, and leaks are tests/test_dev_mem.py's business."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu


def _same(got, ref):
    """bit for bit, every output of a call"""
    got, ref = (x if isinstance(x, (tuple, list)) else (x,) for x in (got, ref))
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        if a is None or b is None:
            assert a is None and b is None, k
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, float(np.nanmax(np.abs(a - b))))


def _first(case, S):
    """the case with its first S posterior samples (the data are the same)"""
    c = dict(case, S=S)
    for k in ("U", "uyLS", "xyLS", "tyLS", "yNoise", "yScale"):
        if c[k] is not None:
            c[k] = np.asfortranarray(c[k][..., :S])
    return c


def _obj(gp, case, S, ctx=None, setup=None):
    """a GPSLCObject of the first S samples on `ctx`, or on a fresh context of its own that `setup` has tuned"""
    o = cases.gpslc_object(gp, _first(case, S))
    if ctx is not None:
        o._ctx = ctx
    elif setup is not None:
        setup(o.ctx())
    return o


def _tasks(ctx):
    ctx.set_task_schedule(min_matrices=1)       # the persistent launch for every chunk, however few matrices


def _profiled(gp, case, setup):
    """a context with the case's data that counts its launches (GPSLC_FLAG_PROFILE: the event pairs are owned resources too)"""
    ctx = gp.Context(case["n"], case["X"].shape[1], case["U"].shape[1], profile=True)
    ctx.set_data(case["X"], case["T"], case["Y"])
    setup(ctx)
    return ctx


def _task_launches(ctx):
    return ctx.profile_get(4)[0]                 # kernel class 4: the persistent factorisation launch


@pytest.fixture(scope="module")
def case300():
    return cases.make_case(300, "UX", False, S=64, seed=11)


def _two_streams(ctx):
    _tasks(ctx)
    ctx.set_tuning(max_batch=32, n_streams=2)


@pytest.mark.parametrize("setup,sizes", [(_tasks, (8, 64, 8)), (_two_streams, (8, 40, 64, 8))], ids=["one-stream", "two-streams"])
def test_slot_arenas_and_progress_words_grow_and_are_reused(gp, case300, setup, sizes):
    def call(o):
        return gp.predict(o, case300["doTs"], want_mean_ite=True)
    ctx = _profiled(gp, case300, setup)
    last = None
    for S in sizes:
        last = call(_obj(gp, case300, S, ctx=ctx))
    chunk = 32 if setup is _two_streams else max(sizes)
    assert _task_launches(ctx) == sum(-(-S // chunk) for S in sizes)       # every chunk took the persistent launch
    _same(last, call(_obj(gp, case300, sizes[-1], setup=setup)))


def test_task_list_cache_evicts_and_rebuilds(gp, case300):
    shapes = [(S, back) for S in (2, 3, 4, 5, 6) for back in (False, True)][:9]

    def call(o, back):
        return gp.predict(o, case300["doTs"], want_mean_ite=back)      # MeanITE needs alpha: the list ends with the back-substitution
    ctx = _profiled(gp, case300, _tasks)
    for S, back in shapes:
        call(_obj(gp, case300, S, ctx=ctx), back)
    assert _task_launches(ctx) == len(shapes)
    S, back = shapes[0]                          # evicted by the ninth shape
    _same(call(_obj(gp, case300, S, ctx=ctx), back), call(_obj(gp, case300, S, setup=_tasks), back))


def test_scratch_of_a_draws_only_call(gp):
    case = cases.make_case(40, "UX", False, S=16, seed=12)

    def call(o):
        return gp.predict(o, case["doTs"], spp=2, seed=5, want_draws=True)      # no MeanITE asked: it lives in the scratch
    ctx = _obj(gp, case, 4).ctx()
    for S in (4, 16):
        call(_obj(gp, case, S, ctx=ctx))
    got = call(_obj(gp, case, 4, ctx=ctx))
    assert got[2] is None
    _same(got, call(_obj(gp, case, 4)))


def _nodes(n, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        nF = (3, 1, 8, 0)[i % 4]
        F = None if nF == 0 else rng.standard_normal((n, nF))
        ls = None if nF == 0 else rng.uniform(0.8, 2.5, nF)
        out.append((F, ls, rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.5), rng.standard_normal(n)))
    return out


def test_scratch_of_the_mid_size_node_kernel(gp):
    nodes = _nodes(300, 8, seed=13)
    ctx = gp.Context(300, 0, 0)
    for count in (2, 8):
        gp.nodesLogpdf(nodes[:count], ctx)
    _same(gp.nodesLogpdf(nodes[:2], ctx), gp.nodesLogpdf(nodes[:2], gp.Context(300, 0, 0)))


def test_pinned_staging_grows_and_serves_the_gradient_launch(gp):
    nodes = [nd for nd in _nodes(40, 67, seed=14) if nd[0] is not None]      # RBF nodes: the gradient launch takes them all
    assert len(nodes) >= 50
    ctx = gp.Context(40, 0, 0)
    for count in (2, 50):
        gp.nodesLogpdf(nodes[:count], ctx)
    fresh = gp.Context(40, 0, 0)
    _same(gp.nodesLogpdf(nodes[:2], ctx), gp.nodesLogpdf(nodes[:2], fresh))
    got, ref = gp.nodesLogpdfGrad(nodes[:2], ctx), gp.nodesLogpdfGrad(nodes[:2], gp.Context(40, 0, 0))
    for g, r in zip(got, ref):
        assert list(g) == list(r)
        _same([np.asarray(v) for v in g.values()], [np.asarray(v) for v in r.values()])


def test_staging_pool_chains_merges_and_settles(gp):
    case = cases.make_case(300, "UX", False, S=512, nU=2, seed=15)
    assert case["U"][:, :, :512].nbytes > (1 << 20)
    ctx = _obj(gp, case, 4).ctx()
    out = [gp.yLogpdf(_obj(gp, case, S, ctx=ctx)) for S in (4, 512, 4, 4)]
    ref = gp.yLogpdf(_obj(gp, case, 4))
    _same(out[2], ref)      # on the merged block
    _same(out[3], ref)      # steady state
    _same(out[1], gp.yLogpdf(_obj(gp, case, 512)))      # and the call that chained


def _cov(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n + 8))
    return A @ A.T / n + np.eye(n)


def test_mvn_cache_across_both_paths(gp):
    n, few, many = 300, 3, 513                   # more than 512 vectors: the tiled path
    rng = np.random.default_rng(16)
    c1, c2 = _cov(n, 1), _cov(n, 2)
    x = rng.standard_normal((n, many))
    sc = rng.uniform(0.5, 2.0, many)
    ctx = gp.Context(n, 0, 0)
    gp.mvnLogpdf(c1, x[:, :few], sc[:few], ctx=ctx)             # single-workgroup path: the dense copy alone
    gp.mvnLogpdf(None, x, sc, ctx=ctx)                          # tiled: the factor is built from the dense copy
    gp.mvnLogpdf(c2, x[:, :few], sc[:few], ctx=ctx)             # the factor is now one hand-over behind
    got = (gp.mvnLogpdf(None, x[:, :few], sc[:few], ctx=ctx), gp.mvnLogpdf(None, x, sc, ctx=ctx),
           gp.mvnDraw(None, x[:, :few], sc[:few], ctx=ctx), gp.mvnDraw(None, x, sc, ctx=ctx))
    a, b = gp.Context(n, 0, 0), gp.Context(n, 0, 0)
    ref = (gp.mvnLogpdf(c2, x[:, :few], sc[:few], ctx=a), gp.mvnLogpdf(c2, x, sc, ctx=b),
           gp.mvnDraw(None, x[:, :few], sc[:few], ctx=a), gp.mvnDraw(None, x, sc, ctx=b))
    _same(got, ref)


def test_mvn_cache_where_the_tiled_factor_is_all_there_is(gp):
    n, S = 700, 4
    rng = np.random.default_rng(17)
    c1, c2 = _cov(n, 3), _cov(n, 4)
    x = rng.standard_normal((n, 150))
    ctx = gp.Context(n, 0, 0)
    gp.mvnLogpdf(c1, x[:, :S], ctx=ctx)
    gp.mvnLogpdf(None, x, ctx=ctx)               # two tile rows of vectors: the staging pool grows under the cached factor
    gp.mvnLogpdf(c2, x[:, :S], ctx=ctx)
    got = (gp.mvnLogpdf(None, x[:, :S], ctx=ctx), gp.mvnDraw(None, x[:, :S], ctx=ctx))
    fresh = gp.Context(n, 0, 0)
    _same(got, (gp.mvnLogpdf(c2, x[:, :S], ctx=fresh), gp.mvnDraw(None, x[:, :S], ctx=fresh)))


def test_create_use_destroy_twenty_times(gp, case300):
    first = None
    for cycle in range(20):
        o = _obj(gp, case300, 8, setup=_tasks)
        out = gp.predict(o, case300["doTs"], want_mean_ite=True)
        o.ctx().close()
        if first is None:
            first = out
        _same(out, first)
