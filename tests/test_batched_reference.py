"""tests/batched_reference.py (the host reference the bench-scale GPU suite checks thousands of posterior samples against)
pinned to the oracle it restates: oracle.structured_sate / structured_ite per sample at 1e-12, and one sample against the
LITERAL restatement (ite_distributions + conditional_sate); node_scores / mvn_scores against orc.mvnormal_logpdf of
orc.process_cov and numpy's Cholesky."""
import numpy as np
import pytest

import batched_reference as br
import cases
import gpslc_oracle as orc

RTOL = 1e-12


def _case(n, binary, L, S=5):
    c = cases.make_case(n, "UX", binary, S=S, seed=n + 7 * L + binary)
    doTs = np.array([0.0, 1.0, 1.0])[:L] if binary else np.linspace(-0.6, 0.9, L)
    return c, doTs


@pytest.mark.parametrize("n", [129, 300, 1000])
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("L", [1, 3])
def test_batched_reference_equals_the_structured_oracle(n, binary, L):
    c, doTs = _case(n, binary, L)
    S = c["S"]
    which = [S - 1, 0, 2]                       # out of order and not all samples: the result follows `samples`
    out = br.structured_batch(c["X"], c["T"], c["Y"], c, which, doTs, ite_samples=[0, S - 1])
    smp = cases.samples_of(c)
    for j, s in enumerate(which):
        rm, rv, logdet, quad = orc.structured_sate(smp[s], c["X"], c["T"], c["Y"], doTs)
        np.testing.assert_allclose(out["meanSATE"][j], rm, rtol=RTOL, atol=0)
        np.testing.assert_allclose(out["varSATE"][j], rv, rtol=RTOL, atol=0)
        np.testing.assert_allclose(out["logdet"][j], logdet, rtol=RTOL, atol=0)
        np.testing.assert_allclose(out["quad"][j], quad, rtol=RTOL, atol=0)
        np.testing.assert_allclose(out["logpdf"][j], -0.5 * (n * np.log(2 * np.pi) + logdet + quad), rtol=RTOL, atol=0)
        if s in (0, S - 1):
            for l in range(L):
                m, _ = orc.structured_ite(smp[s], c["X"], c["T"], c["Y"], doTs[l])
                assert np.max(np.abs(out["meanITE"][s][:, l] - m)) <= RTOL * np.max(np.abs(m))
        else:
            assert s not in out["meanITE"]


def test_batched_reference_chunks_and_model_shapes(monkeypatch):
    """Several chunks in one call (a tiny chunk budget), and the shapes without U or without X."""
    monkeypatch.setattr(br, "CHUNK_BYTES", 2 * 8 * 200 * 200)
    for shape in ("UX", "U", "X", "T"):
        c = cases.make_case(200, shape, False, S=5, seed=11)
        doTs = np.array([-0.3, 0.4])
        out = br.structured_batch(c["X"], c["T"], c["Y"], c, range(5), doTs, ite_samples=[3])
        for s, p in enumerate(cases.samples_of(c)):
            rm, rv, logdet, quad = orc.structured_sate(p, c["X"], c["T"], c["Y"], doTs)
            np.testing.assert_allclose(out["meanSATE"][s], rm, rtol=RTOL, atol=0)
            np.testing.assert_allclose(out["varSATE"][s], rv, rtol=RTOL, atol=0)
            np.testing.assert_allclose(out["logdet"][s] + out["quad"][s], logdet + quad, rtol=RTOL, atol=0)
        m, _ = orc.structured_ite(cases.samples_of(c)[3], c["X"], c["T"], c["Y"], doTs[1])
        assert np.max(np.abs(out["meanITE"][3][:, 1] - m)) <= RTOL * np.max(np.abs(m))


def test_batched_reference_against_the_literal_restatement():
    """One sample against the reference algorithm as written (5 log-kernels, three symmetric-indefinite solves, four block
    products: src/likelihood.jl:8-52, src/estimation.jl:36-50, 116-121) and its :Y log-density (y_logpdf)."""
    c, doTs = _case(300, False, 2, S=3)
    s = 1
    p = cases.samples_of(c)[s]
    out = br.structured_batch(c["X"], c["T"], c["Y"], c, [s], doTs, ite_samples=[s])
    for l, doT in enumerate(doTs):
        M, Cv = orc.ite_distributions([p], c["X"], c["T"], c["Y"], doT)
        rm, rv = orc.conditional_sate(M[0], Cv[0])
        assert abs(out["meanSATE"][0, l] - rm) <= 1e-9 * abs(rm)
        assert abs(out["varSATE"][0, l] - rv) <= 1e-9 * abs(rv)
        assert np.max(np.abs(out["meanITE"][s][:, l] - M[0])) <= 1e-9 * np.max(np.abs(M[0]))
    lp = orc.y_logpdf(p.uyLS, p.xyLS, p.tyLS, p.yScale, p.yNoise, p.U, c["X"], c["T"], c["Y"])
    assert abs(out["logpdf"][0] - lp) <= 1e-10 * abs(lp)


def _nodes(n, nFs, seed):
    rng = np.random.default_rng(seed)
    nodes = []
    for nF in nFs:
        F = None if nF == 0 else rng.standard_normal((n, nF))
        ls = None if nF == 0 else rng.uniform(0.6, 2.0, nF)
        nodes.append((F, ls, rng.uniform(0.5, 2.0), rng.uniform(0.2, 1.5), rng.standard_normal(n)))
    return nodes


@pytest.mark.parametrize("n", [1, 17, 150, 300])
def test_node_scores_equal_the_oracle(n, monkeypatch):
    """Heterogeneous feature counts (0 .. 32) in one call, over several chunks, against orc.mvnormal_logpdf(process_cov(...))
    and numpy's Cholesky; a node that is not positive definite gets LAPACK's info and NaN, the others are unaffected."""
    monkeypatch.setattr(br, "CHUNK_BYTES", 3 * 8 * n * n)
    nodes = _nodes(n, (0, 1, 3, 8, 16, 32, 2), seed=n)
    F, ls, sc, _, tg = nodes[3]
    nodes.append((F, ls, sc, -sc - 1.0, tg))                  # diagonal sc + noise = -1: fails at the first pivot
    out = br.node_scores(nodes)
    for i, (F, ls, sc, nz, tg) in enumerate(nodes[:-1]):
        K = sc * np.ones((n, n)) + nz * np.eye(n) if F is None else orc.process_cov(orc.rbf_kernel_log(F, F, ls), sc, nz)
        np.testing.assert_allclose(out["logpdf"][i], orc.mvnormal_logpdf(tg, K), rtol=RTOL, atol=0)
        ref = np.linalg.cholesky(K) @ tg
        assert np.max(np.abs(out["draw"][:, i] - ref)) <= RTOL * np.max(np.abs(ref)), i
        assert out["info"][i] == 0
    assert out["info"][-1] == 1 and np.isnan(out["logpdf"][-1]) and np.isnan(out["draw"][:, -1]).all()


@pytest.mark.parametrize("n,S", [(1, 3), (150, 7), (300, 40)])
def test_mvn_scores_equal_the_oracle(n, S, monkeypatch):
    monkeypatch.setattr(br, "CHUNK_BYTES", 8 * 8 * n)        # several column chunks
    rng = np.random.default_rng(100 + n)
    G = rng.standard_normal((n, n))
    cov = G @ G.T / n + np.eye(n)
    X = rng.standard_normal((n, S))
    cs = rng.uniform(0.3, 3.0, S)
    out = br.mvn_scores(cov, X, cs)
    L = np.linalg.cholesky(cov)
    for s in range(S):
        np.testing.assert_allclose(out["logpdf"][s], orc.mvnormal_logpdf(X[:, s], cs[s] * cov), rtol=RTOL, atol=0)
        ref = np.sqrt(cs[s]) * (L @ X[:, s])
        assert np.max(np.abs(out["draw"][:, s] - ref)) <= RTOL * np.max(np.abs(ref)), s
    one = br.mvn_scores(cov, X)
    np.testing.assert_allclose(one["logpdf"], [orc.mvnormal_logpdf(X[:, s], cov) for s in range(S)], rtol=RTOL, atol=0)
    bad = cov.copy()
    bad[n // 2, n // 2] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        br.mvn_scores(bad, X)


# ---- unit B / C: ITE covariances and draws of (sample, level) pairs ---------------------------------------------------------

def _pairs_case(n, L, S=3, seed=0):
    c = cases.make_case(n, "UX", False, S=S, seed=seed)
    return c, np.linspace(-0.8, 1.1, L)


@pytest.mark.parametrize("n", [129, 300])
def test_ite_pairs_equal_the_structured_and_literal_oracle(n, monkeypatch):
    """ite_pairs against orc.structured_ite (1e-12, the same formulas) and orc.ite_distributions (the literal restatement:
    three symmetric-indefinite solves; 1e-9) for pairs out of order and over several chunks; a ragged n."""
    monkeypatch.setattr(br, "CHUNK_BYTES", 2 * 8 * n * n)
    c, doTs = _pairs_case(n, 3)
    pn = 1e-3
    pairs = [(2, 1), (0, 0), (1, 2), (2, 0), (0, 2)]
    out = br.ite_pairs(c["X"], c["T"], c["Y"], c, pairs, doTs, pn)
    smp = cases.samples_of(c)
    for j, (s, l) in enumerate(pairs):
        m, C = orc.structured_ite(smp[s], c["X"], c["T"], c["Y"], doTs[l])
        C = orc._symmetric_upper(C) + pn * np.eye(n)
        assert np.max(np.abs(out["mean"][j] - m)) <= RTOL * np.max(np.abs(m)), (s, l)
        assert np.max(np.abs(out["cov"][j] - C)) <= RTOL * np.max(np.abs(C)), (s, l)
        assert np.array_equal(out["cov"][j], out["cov"][j].T)
        M, Cv = orc.ite_distributions([smp[s]], c["X"], c["T"], c["Y"], doTs[l], pn)
        assert np.max(np.abs(out["mean"][j] - M[0])) <= 1e-9 * np.max(np.abs(M[0])), (s, l)
        assert np.max(np.abs(out["cov"][j] - Cv[0])) <= 1e-9 * np.max(np.abs(Cv[0])), (s, l)


def test_ite_pairs_vector_levels_equal_the_vector_restatement():
    """(L, n) intervention vectors: against vector_restatement.ite_distributions_vec (the literal formula with d in place of
    fill(doT, n)); and a constant vector gives the scalar level's result."""
    import vector_restatement as vr
    n = 150
    c, _ = _pairs_case(n, 2, seed=3)
    D = vr.policy(c, 2, seed=5)
    pn = 1e-3
    pairs = [(0, 1), (2, 0)]
    out = br.ite_pairs(c["X"], c["T"], c["Y"], c, pairs, D, pn)
    smp = cases.samples_of(c)
    for j, (s, l) in enumerate(pairs):
        M, Cv = vr.ite_distributions_vec([smp[s]], c["X"], c["T"], c["Y"], D[l], pn)
        assert np.max(np.abs(out["mean"][j] - M[0])) <= 1e-9 * np.max(np.abs(M[0])), (s, l)
        assert np.max(np.abs(out["cov"][j] - Cv[0])) <= 1e-9 * np.max(np.abs(Cv[0])), (s, l)
    flat = br.ite_pairs(c["X"], c["T"], c["Y"], c, [(1, 0)], np.full((1, n), 0.3), pn)
    scal = br.ite_pairs(c["X"], c["T"], c["Y"], c, [(1, 0)], np.array([0.3]), pn)
    assert np.max(np.abs(flat["cov"] - scal["cov"])) <= RTOL * np.max(np.abs(scal["cov"]))
    assert np.max(np.abs(flat["mean"] - scal["mean"])) <= RTOL * np.max(np.abs(scal["mean"]))


def test_ite_pair_draws_equal_the_oracle_samples(monkeypatch):
    """ite_pair_draws against orc.ite_samples on the same CovITE (1e-12) and its eigenvalue bounds against numpy's; at the
    default jitter against orc.sample_ite (the literal chain) within draw_bounds' conditioning-aware bound."""
    n, spp = 257, 3
    monkeypatch.setattr(br, "CHUNK_BYTES", 2 * 8 * n * n)
    c, doTs = _pairs_case(n, 2, seed=4)
    pairs = [(s, l) for s in range(3) for l in range(2)]
    z = np.random.default_rng(1).standard_normal((len(pairs), n, spp))
    smp = cases.samples_of(c)
    for pn in (1e-3, orc.PREDICTION_COVARIANCE_NOISE):
        ref = br.ite_pairs(c["X"], c["T"], c["Y"], c, pairs, doTs, pn)
        out = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, pairs, doTs, z, pn)
        for j, (s, l) in enumerate(pairs):
            want = orc.ite_samples(ref["mean"][j][None], ref["cov"][j][None], spp, z[j])
            assert np.max(np.abs(out["draws"][j] - want)) <= RTOL * np.max(np.abs(want)), (pn, s, l)
            ev = np.linalg.eigvalsh(ref["cov"][j])
            assert abs(out["lam_max"][j] - ev[-1]) <= 1e-12 * ev[-1]
            assert abs(out["lam_min"][j] - ev[0]) <= 1e-12 * ev[-1]
        if pn == 1e-3:
            continue
        s, l = 1, 0
        lit = orc.sample_ite([smp[s]], c["X"], c["T"], c["Y"], doTs[l], spp, z[pairs.index((s, l))], pn)
        j = pairs.index((s, l))
        ok, worst = br.draws_match(out["draws"][j], lit, out["lam_min"][j], out["lam_max"][j], z[j], tight=False)
        assert ok, worst


def test_first_failing_pivot_is_lapack_info():
    rng = np.random.default_rng(2)
    n = 300
    G = rng.standard_normal((n, n))
    C = G @ G.T / n + 0.1 * np.eye(n)
    assert br.first_failing_pivot(C) == 0
    for p in (1, 128, 129, 300):
        # the leading p-1 block is untouched; pivot p becomes its Schur complement minus 1
        piv, d = br.schur_pivots(C, p)
        assert np.all(piv > 0) and d > 0
        B = C.copy()
        B[p - 1, p - 1] -= d + 1.0
        assert br.first_failing_pivot(B) == p
        piv2, d2 = br.schur_pivots(B, p)
        np.testing.assert_allclose(piv2, piv, rtol=1e-12)
        assert abs(d2 + 1.0) <= 1e-9
    assert list(br.first_failing_pivot(np.stack([C, B]))) == [0, 300]


# The GPU tests hold every draw column of a pair to draw_bounds' tight bound through br.draws_match.  Those tolerances must
# discriminate: each deliberately wrong reference below (a plausible indexing slip of the draw path, restated on the host)
# must fail for every pair it touches.

def _sens_case():
    n, S, L, spp = 383, 3, 3, 4            # nt = 3: a middle tile row (rows 128 .. 255) and a ragged last tile
    c, doTs = _pairs_case(n, L, S=S, seed=8)
    pn = 1e-3
    pairs = [(s, l) for s in range(S) for l in range(L)]
    seed = 17
    z = np.stack([orc.philox_normals(seed, s + S * l, n * spp).reshape(n, spp, order="F") for s, l in pairs])
    ref = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, pairs, doTs, z, pn)
    return c, doTs, pn, pairs, z, ref, seed


@pytest.fixture(scope="module")
def sens():
    return _sens_case()


def test_draw_tolerance_accepts_the_right_reference(sens):
    c, doTs, pn, pairs, z, ref, _ = sens
    for j in range(len(pairs)):
        ok, worst = br.draws_match(ref["draws"][j], ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])
        assert ok and worst == 0.0


def test_draw_tolerance_rejects_a_level_shifted_by_one(sens):
    c, doTs, pn, pairs, z, ref, _ = sens
    L = len(doTs)
    for j, (s, l) in enumerate(pairs):
        wrong = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, [(s, (l + 1) % L)], doTs, z[j:j + 1], pn)["draws"][0]
        assert not br.draws_match(wrong, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])[0], (s, l)


def test_draw_tolerance_rejects_the_philox_stream_of_the_next_sample(sens):
    c, doTs, pn, pairs, z, ref, seed = sens
    n, spp = z.shape[1], z.shape[2]
    S = c["S"]
    for j, (s, l) in enumerate(pairs):
        zw = orc.philox_normals(seed, (s + 1) + S * l, n * spp).reshape(1, n, spp, order="F")
        wrong = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, [(s, l)], doTs, zw, pn)["draws"][0]
        assert not br.draws_match(wrong, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])[0], (s, l)


def test_draw_tolerance_rejects_a_lost_middle_tile_row(sens):
    """The middle tile row of nt = 3 (no partner row in the streaming draw kernel) left at the mean: L_c z dropped there."""
    c, doTs, pn, pairs, z, ref, _ = sens
    means = br.ite_pairs(c["X"], c["T"], c["Y"], c, pairs, doTs, pn)["mean"]
    for j in range(len(pairs)):
        wrong = ref["draws"][j].copy()
        wrong[128:256] = means[j][128:256, None]
        assert not br.draws_match(wrong, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])[0], pairs[j]


def test_draw_tolerance_rejects_a_later_sub_batch_from_the_previous_sample(sens):
    """A later sub-batch (sample group g0 > 0) written with the previous sample's draws: its own normals, the wrong
    sample's MeanITE and factor."""
    c, doTs, pn, pairs, z, ref, _ = sens
    for j, (s, l) in enumerate(pairs):
        if s == 0:
            continue
        wrong = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, [(s - 1, l)], doTs, z[j:j + 1], pn)["draws"][0]
        assert not br.draws_match(wrong, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])[0], (s, l)
        prev = ref["draws"][pairs.index((s - 1, l))]
        assert not br.draws_match(prev, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], z[j])[0], (s, l)
