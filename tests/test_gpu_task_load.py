"""The persistent factorisation launch (potrf_tasks_kernel) at the DEFAULT schedule and at bench scale, against the oracle.

Since the launch needs >= 256 matrices per chunk (gpslc_ctx::task_min_batch), the oracle-parity suites at S <= 48 run the
per-column schedule, and tests/test_gpu_tasks.py forces the launch down to a few dozen matrices.  Here the calls are the bench's
own shapes — 8,192 matrices at N = 1024 in one launch (1,024 per XCD queue), 1,024 at N = 4096 — where the tile hand-off
between workgroups (release / acquire on per-matrix progress words) runs with every workgroup slot live and HBM saturated.  A
stale read is timing-dependent and touches single matrices, so:
  * every sample is checked through size-independent properties (mean_i MeanITE_i == MeanSATE: two code paths; VarSATE finite
    and > 0; no failed pivot);
  * hundreds of samples — the first and last matrix of each queue run, both sides of group boundaries inside the runs, seeded
    random ones — are checked against the structured restatement (tests/batched_reference.py) at test_gpu_fullsize's tolerances;
  * the launch is compared bit for bit with the per-column schedule, repeated, with two launches in flight (two streams; two
    contexts of gpslc_predict_multi), and at the edges of the default thresholds.
No test changes the schedule of the run it measures; each one asserts from the profile counters which schedule ran (a later
change of the thresholds cannot silently send these tests back to the per-column path).  Contexts are closed explicitly: one
context's chunk arenas at N = 4096 take ~28 % of the device.
"""
import os

import numpy as np
import pytest

import batched_reference as br
import gpslc_oracle as orc

pytestmark = pytest.mark.gpu

TASK_GROUP = 32          # matrices per group of the task order (gpslc_ctx::task_group's default; task_list.h)
PROF_TASKS = 4           # profile class of the persistent launch (potrf_tasks)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _data(gp, n, D, K, S, binary=False, seed=1234):
    X, T, Y, objid = gp.synth.make_dataset(n, D, binary_t=binary, seed=seed)
    post = gp.synth.make_posterior(n, D, K, S, objid, seed=seed)
    return X, T, Y, post


def _subset(post, k):
    """the first k posterior samples of a pack"""
    out = {}
    for key, v in post.items():
        out[key] = None if v is None else np.asfortranarray(v[..., :k])
    return out


def _obj(gp, data, n_streams=0, max_batch=0):
    """a GPSLCObject whose context records HIP events (which schedule ran: profile_get(PROF_TASKS))"""
    X, T, Y, post = data
    g = gp.GPSLCObject(X, T, Y, post["U"], post["uyLS"], post["xyLS"], post["tyLS"], post["yNoise"], post["yScale"])
    g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)
    g._ctx.set_data(g.X, g.T, g.Y)
    if n_streams or max_batch:
        g._ctx.set_tuning(max_batch, 0, n_streams)
    return g


def _run(gp, g, doTs, logpdf=True):
    """predict (+ yLogpdf) on g's context; returns (ms, vs, mi, lp, info, persistent launches)"""
    ctx = g.ctx()
    ctx.profile_reset()
    ms, vs, mi = gp.predict(g, doTs, want_mean_ite=True)
    info = ctx.last_info(g.getNumPosteriorSamples())
    lp = gp.yLogpdf(g) if logpdf else None
    return ms, vs, mi, lp, info, ctx.profile_get(PROF_TASKS)[0]


def _per_column(gp, g, doTs, logpdf=True):
    """the same call on the same context with the persistent launch switched off"""
    g.ctx().set_task_schedule(2, 0)
    out = _run(gp, g, doTs, logpdf)
    assert out[5] == 0
    return out


def _close(g):
    if g._ctx is not None:
        g._ctx.close()
    for cs in g.__dict__.get("_multi", {}).values():
        for c in cs:
            c.close()


def _same(a, b, what=""):
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[:4].tolist()}")


def _same_outputs(x, y):
    for k, name in enumerate(("meanSATE", "varSATE", "MeanITE", "logpdf")):
        if x[k] is not None and y[k] is not None:
            _same(x[k], y[k], name)


def _every_sample(ms, vs, mi, info):
    """size-independent checks of every posterior sample"""
    assert not info.any(), np.flatnonzero(info)[:8]
    assert np.all(np.isfinite(ms)) and np.all(np.isfinite(vs)) and np.all(vs > 0)
    err = np.abs(mi.mean(axis=0) - ms)
    bound = 1e-10 * np.max(np.abs(ms)) + 1e-13
    assert np.max(err) <= bound, (np.argwhere(err > bound)[:8].tolist(), float(np.max(err)))


def _queue_runs(nb):
    """[x0, x1) of the eight per-XCD queue runs of a chunk of nb matrices (build_task_list, task_list.h)"""
    wq, wrm = nb >> 3, nb & 7
    return [(x * wq + min(x, wrm), x * wq + min(x, wrm) + wq + (1 if x < wrm else 0)) for x in range(8)]


def _run_edges(nb):
    return sorted({s for x0, x1 in _queue_runs(nb) if x1 > x0 for s in (x0, x1 - 1)})


def _group_edges(nb, stride):
    """both sides of every stride-th group boundary inside each queue run"""
    out = set()
    for x0, x1 in _queue_runs(nb):
        for b in range(x0 + TASK_GROUP, x1, TASK_GROUP * stride):
            out.update((b - 1, b))
    return sorted(out)


def _check_vs_reference(ref, which, ms, vs, mi, lp, post, ite=()):
    """test_gpu_fullsize._check_vs_structured's tolerances, for the samples `which` (ref = br.structured_batch over them)"""
    for j, s in enumerate(which):
        rm, rv = ref["meanSATE"][j], ref["varSATE"][j]
        ysc = float(post["yScale"][s])
        assert np.all(np.abs(ms[s] - rm) <= 1e-6 * np.abs(rm) + 1e-12), (s, ms[s], rm)      # north-star tolerance
        assert np.all(np.abs(vs[s] - rv) <= 1e-6 * np.abs(rv) + 1e-9 * ysc), (s, vs[s], rv)
        assert np.all(np.abs(ms[s] - rm) <= 1e-9 * np.abs(rm) + 1e-13), (s, ms[s], rm)      # what fp64 delivers
        if lp is not None:
            assert abs(lp[s] - ref["logpdf"][j]) <= 1e-10 * abs(ref["logpdf"][j]), (s, lp[s], ref["logpdf"][j])
    for s in ite:
        m = ref["meanITE"][s]
        for l in range(m.shape[1]):
            assert np.max(np.abs(mi[:, s, l] - m[:, l])) <= 1e-8 * np.max(np.abs(m[:, l])) + 1e-13, (s, l)


def _sample(post, s):
    return orc.PosteriorSample(None if post["uyLS"] is None else post["uyLS"][:, s],
                               None if post["xyLS"] is None else post["xyLS"][:, s],
                               float(post["tyLS"][s]), float(post["yNoise"][s]), float(post["yScale"][s]),
                               None if post["U"] is None else post["U"][:, :, s])


# ---- a. BASELINE config 2 at bench scale: N = 1024, D = 4, nU = 1, S = 8192 in ONE persistent launch ---------------------------
C2 = dict(n=1024, D=4, K=1, S=8192)


@pytest.fixture(scope="module")
def c2(gp):
    """one default call at config 2 (kept as host arrays; its context is closed)"""
    data = _data(gp, C2["n"], C2["D"], C2["K"], C2["S"])
    doTs = gp.synth.levels(data[1], 1)
    g = _obj(gp, data)
    try:
        out = _run(gp, g, doTs)
    finally:
        _close(g)
    return data, doTs, out


def _c2_samples(S):
    edges = _run_edges(S)
    groups = _group_edges(S, stride=3)
    rest = sorted(set(range(S)) - set(edges) - set(groups))
    rnd = np.random.default_rng(2024).choice(rest, size=max(0, 256 - len(edges) - len(groups)), replace=False)
    return edges, sorted(set(edges) | set(groups) | set(int(s) for s in rnd))


def test_config2_bench_scale_every_sample_and_the_reference(gp, c2):
    (X, T, Y, post), doTs, (ms, vs, mi, lp, info, launches) = c2
    S = C2["S"]
    assert launches > 0                                                 # the default schedule ran the persistent launch
    _every_sample(ms, vs, mi, info)
    edges, which = _c2_samples(S)
    assert len(which) >= 256 and len(edges) == 16
    ite = edges[::2]                                                    # the first matrix of every queue run
    ref = br.structured_batch(X, T, Y, post, which, doTs, ite_samples=ite)
    _check_vs_reference(ref, which, ms, vs, mi, lp, post, ite=ite)
    # one unit against the LITERAL restatement (5 kernels, 3 Bunch-Kaufman solves, 4 GEMMs): the last matrix of queue 3
    s = _queue_runs(S)[3][1] - 1
    p = _sample(post, s)
    M, Cv = orc.ite_distributions([p], X, T, Y, float(doTs[0]))
    rm, rv = orc.conditional_sate(M[0], Cv[0])
    assert abs(ms[s, 0] - rm) <= 1e-6 * abs(rm) + 1e-12
    assert abs(vs[s, 0] - rv) <= 1e-6 * abs(rv) + 1e-9 * p.yScale
    assert np.max(np.abs(mi[:, s, 0] - M[0])) <= 1e-6 * np.max(np.abs(M[0])) + 1e-12


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("GPSLC_RUN_SLOW") != "1",
                    reason="set GPSLC_RUN_SLOW=1: all 8,192 samples against the host reference take minutes of host CPU")
def test_config2_bench_scale_all_samples_against_the_reference(gp, c2):
    (X, T, Y, post), doTs, (ms, vs, mi, lp, info, launches) = c2
    assert launches > 0
    which = list(range(C2["S"]))
    ref = br.structured_batch(X, T, Y, post, which, doTs)
    _check_vs_reference(ref, which, ms, vs, mi, lp, post)


# ---- b. BASELINE config 3 at bench scale: N = 4096, D = 8, nU = 2, S = 1024 in ONE persistent launch ---------------------------
def test_config3_bench_scale_every_sample_and_the_reference(gp):
    n, D, K, S = 4096, 8, 2, 1024
    data = _data(gp, n, D, K, S)
    X, T, Y, post = data
    doTs = gp.synth.levels(T, 1)
    g = _obj(gp, data)
    try:
        ms, vs, mi, lp, info, launches = _run(gp, g, doTs)
    finally:
        _close(g)
    assert launches > 0
    _every_sample(ms, vs, mi, info)
    which = _run_edges(S)
    assert len(which) == 16
    ref = br.structured_batch(X, T, Y, post, which, doTs)
    _check_vs_reference(ref, which, ms, vs, mi, lp, post)


# ---- c. bit-identity with the per-column schedule at bench scale, three launches on one context --------------------------------
@pytest.mark.parametrize("n,D,K,S", [(1024, 4, 1, 8192), (4096, 8, 2, 1024)])
def test_bench_scale_launch_is_repeatable_and_equals_the_per_column_schedule(gp, n, D, K, S):
    data = _data(gp, n, D, K, S)
    doTs = gp.synth.levels(data[1], 1)
    g = _obj(gp, data)
    try:
        runs = []
        for _ in range(3):
            out = _run(gp, g, doTs)
            assert out[5] > 0
            runs.append(out)
        col = _per_column(gp, g, doTs)
    finally:
        _close(g)
    _every_sample(*col[:3], col[4])
    for out in runs:
        _same_outputs(out, col)


# ---- d. two persistent launches in flight -------------------------------------------------------------------------------------
def test_two_streams_with_two_launches_in_flight(gp, c2):
    """max_batch 2048 over two streams: four chunks of 2,048 matrices, two persistent launches running at once (one per stream
    slot, each with its own progress words) — bit-identical to the single-stream call of 8,192 matrices in one launch."""
    data, doTs, ref = c2
    g = _obj(gp, data, n_streams=2, max_batch=2048)
    try:
        out = _run(gp, g, doTs, logpdf=False)
    finally:
        _close(g)
    assert out[5] == 4
    _same_outputs(out, ref[:3] + (None,))


def test_predict_multi_two_contexts_on_one_gpu(gp, c2):
    """gpslc_predict_multi over devices [0, 0]: two contexts of 512 matrices each, each with its persistent launch, driven from
    two host threads — bit-identical to one context's call."""
    (X, T, Y, post), doTs, _ = c2
    data = (X, T, Y, _subset(post, 1024))
    single = _obj(gp, data)
    try:
        one = _run(gp, single, doTs, logpdf=False)
    finally:
        _close(single)
    assert one[5] > 0
    ms8, vs8, mi8 = c2[2][:3]
    _same_outputs(one, (ms8[:1024], vs8[:1024], mi8[:, :1024], None))
    g = gp.GPSLCObject(X, T, Y, *(data[3][k] for k in ("U", "uyLS", "xyLS", "tyLS", "yNoise", "yScale")))
    cs = []
    for _ in range(2):
        c = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=True)
        c.set_data(g.X, g.T, g.Y)
        c.profile_reset()
        cs.append(c)
    g.__dict__["_multi"] = {(0, 0): cs}
    try:
        ms, vs, mi = gp.predict(g, doTs, want_mean_ite=True, devices=[0, 0])
        launches = [c.profile_get(PROF_TASKS)[0] for c in cs]
    finally:
        _close(g)
    assert all(v > 0 for v in launches), launches
    _same_outputs((ms, vs, mi, None), one)


# ---- e. edges at the default thresholds ---------------------------------------------------------------------------------------
def test_255_matrices_take_the_per_column_schedule_256_the_launch(gp, c2):
    (X, T, Y, post), doTs, ref = c2
    for S, launched in ((255, False), (256, True)):
        g = _obj(gp, (X, T, Y, _subset(post, S)))
        try:
            out = _run(gp, g, doTs)
        finally:
            _close(g)
        assert (out[5] > 0) == launched, (S, out[5])
        _same_outputs(out, (ref[0][:S], ref[1][:S], ref[2][:, :S], ref[3][:S]))


@pytest.mark.parametrize("n,D,K,L,binary", [
    (1000, 4, 1, 1, False),          # partial last tile, 8 tiles per side
    (4000, 8, 2, 1, False),          # partial last tile, 32 tiles per side
    (1024, 4, 1, 40, False),         # > 32 right-hand sides: the augmented row is a full tile row of the task list
    (1024, 4, 1, 2, True),           # binary T
])
def test_default_launch_edges_against_the_reference_and_the_per_column_schedule(gp, n, D, K, L, binary):
    S = 256
    data = _data(gp, n, D, K, S, binary=binary, seed=4321 + n + L)
    X, T, Y, post = data
    doTs = np.array([0.0, 1.0]) if binary else gp.synth.levels(T, L)
    g = _obj(gp, data)
    try:
        out = _run(gp, g, doTs)
        assert out[5] > 0
        col = _per_column(gp, g, doTs)
    finally:
        _close(g)
    _every_sample(*out[:3], out[4])
    _same_outputs(out, col)
    which = _run_edges(S) if n <= 1024 else _run_edges(S)[::2]
    ite = which[:2] if n <= 1024 else ()
    ref = br.structured_batch(X, T, Y, post, which, doTs, ite_samples=ite)
    _check_vs_reference(ref, which, *out[:4], post, ite=ite)


def test_a_call_whose_chunks_straddle_the_threshold(gp):
    """N = 4096, S = 1100: a chunk of 1,024 matrices through the persistent launch, then 76 (< 256) through the per-column
    schedule — every sample equal to an all-per-column call."""
    n, D, K, S = 4096, 8, 2, 1100
    data = _data(gp, n, D, K, S, seed=99)
    doTs = gp.synth.levels(data[1], 1)
    g = _obj(gp, data)
    try:
        out = _run(gp, g, doTs, logpdf=False)
        col = _per_column(gp, g, doTs, logpdf=False)
    finally:
        _close(g)
    assert out[5] == 1
    _every_sample(*out[:3], out[4])
    _same_outputs(out, col)
