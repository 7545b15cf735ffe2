"""tests/batched_reference.py (the host reference the bench-scale GPU suite checks thousands of posterior samples against)
pinned to the oracle it restates: oracle.structured_sate / structured_ite per sample at 1e-12, and one sample against the
LITERAL restatement (ite_distributions + conditional_sate)."""
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
