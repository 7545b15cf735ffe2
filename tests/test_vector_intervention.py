"""Per-individual interventions on the host: the dense restatement (tests/vector_restatement.py) against the oracle, its
exact-zero identities, and the Python mirror's Intervention parsing (everything that is decided before a device is used)."""
import numpy as np
import pytest

import cases
import gpslc_oracle as orc
import vector_restatement as vr


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("bt", [False, True])
def test_restatement_reduces_to_the_oracle_for_a_filled_vector(shape, bt):
    c = cases.make_case(24, shape, bt, S=1, seed=3)
    p = cases.samples_of(c)[0]
    for x in c["doTs"]:
        ref = orc.likelihood_distribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], x)
        got = vr.likelihood_distribution_vec(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"],
                                             np.full(24, x))
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
@pytest.mark.parametrize("bt", [False, True])
def test_restatement_exact_zeros_when_the_intervention_is_the_observed_treatment(shape, bt):
    c = cases.make_case(24, shape, bt, S=1, seed=4)
    p = cases.samples_of(c)[0]
    m, C = vr.conditional_ite_vec(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], c["T"])
    assert np.array_equal(m, np.zeros(24)) and np.array_equal(C, np.zeros((24, 24)))
    # a mixed policy: row i of CovWWs' - CovWW vanishes wherever d_i == T_i
    d, same = vr.mixed(c, seed=5)
    assert same.any() and (~same).any()
    m, _ = vr.conditional_ite_vec(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], d)
    assert np.all(m[same] == 0.0)


def _obj(gp, n=12):
    c = cases.make_case(n, "UX", False, S=2, seed=6)
    return c, cases.gpslc_object(gp, c)


def test_intervention_parsing():
    from causalgpslc_jl_amd.api import _intervention
    assert _intervention(0.5, 4) == (0.5, None)
    assert _intervention(True, 4) == (1.0, None)
    assert _intervention(np.float64(2.0), 4) == (2.0, None)
    x, d = _intervention([True, False, True, False], 4)
    assert x is None and d.dtype == np.float64 and np.array_equal(d, [1.0, 0.0, 1.0, 0.0])
    x, d = _intervention(np.arange(4.0), 4)
    assert x is None and np.array_equal(d, np.arange(4.0))
    for bad in (np.zeros(3), np.zeros((4, 1)), [[1.0] * 4]):
        with pytest.raises(ValueError, match="n = 4"):
            _intervention(bad, 4)


def test_public_entry_points_refuse_a_wrong_length_before_any_device_call():
    import causalgpslc_jl_amd as gp
    c, g = _obj(gp)
    bad = np.zeros(c["n"] + 1)
    for f in (gp.SATEDistributions, gp.sampleSATE, gp.sampleITE, gp.ITEDistributions):
        with pytest.raises(ValueError, match=f"n = {c['n']}"):
            f(g, bad)
    with pytest.raises(ValueError, match=f"n = {c['n']}"):
        gp.predict(g, np.zeros((2, c["n"] - 1)))
    p = cases.samples_of(c)[0]
    with pytest.raises(ValueError, match=f"n = {c['n']}"):
        gp.likelihoodDistribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], bad)
    with pytest.raises(ValueError, match=f"n = {c['n']}"):
        gp.conditionalITE(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], bad)
    assert g._ctx is None          # nothing reached a device


def test_vector_levels_are_not_sharded():
    import causalgpslc_jl_amd as gp
    c, g = _obj(gp)
    with pytest.raises(NotImplementedError, match="devices"):
        gp.predict(g, np.tile(c["T"], (2, 1)), devices=[0, 0])
    assert g._ctx is None and not g.__dict__.get("_multi")
