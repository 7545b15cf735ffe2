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
