"""The kernels that evaluate the model's kernel function on pairs of individuals against results recorded BEFORE their front
end was folded into one place: the feature staging (stage_scaled_features, gpslc_internal.h), the tile-build body that
dt_build_kernel (D / Delta of the full ITE covariance) and ld_build_kernel (the likelihood blocks) now share (k_solve.hip), the
lower-triangle tile decode (tri_decode) and the treatment kernel gp_rho (gp_math.h).  The fold keeps every floating-point
operation, its operands and its order — each element depends only on its own row and column, lux is summed in feature order by
fma either way — so every output must be equal BIT FOR BIT; a tolerance has no place here.
tests/golden/tile_build_parent_hashes.json holds the parent commit's hash and the SHA-256 of every output the parent returned on
an MI355X for the seeded cases below (S = 2 wherever the entry point takes samples, so the batch index is nonzero).  Sizes:
n = 128 (one full tile, no padding), 129 (one live row and column in the second tile: the rectangular tiles (0,1) and (1,0), the
identity and zero padding) and 200; feature counts F = 0 (shape T), 1, 5 (an exact Gram instantiation), 7 (the Gram kernel's
runtime-F path) and 32 (MAXF, the LDS opt-in limit).
  1. ITEDistributions (MeanITEs, CovITEs): plain with doT = one T[i] (an exact-zero row), a random intervention vector, a
     contrast a != b, at n in {128, 129, 200} with F = 5 and at n = 129 with F in {0, 1, 7, 32}; at n = 129, F = 5 also the
     vector d == T (every output an exact zero) and the contrast a == b.
  2. likelihoodDistribution, all seven blocks, scalar and vector doT, at n in {128, 129, 200} with F = 5 and at n = 129 with
     F in {0, 32} (the entry point takes one parameter set: the case's second sample).
  3. Unit B through predict with draws: n = 129, L = 3, spp = 2, seeded, plain / vector / contrast (the b / lc, b % lc, l0
     indexing of dt_build_kernel).  No gpslc_set_tuning makes l0 > 0 at this size (a sub-batch holds min(128, Bt L) >= L
     pairs, predict.hip), so there is no split case.
  4. The VALU MeanITE ladder (predict(want_mean_ite=True), n = 200): fp64 at L = 1 and 2 with F in {3, 5, 6, 7, 9, 11, 14, 18,
     32} (rungs 4, 5, 6, 8, 10, 12, 16, 20, 32), a contrast at F = 5, L = 2, and fp32_kernel at F = 5 and 14 with L = 2 and
     L = 17 (the 16-level VALU path; F = 14 takes the float runtime-F Gram path).
  5. Vector levels through predict: n = 129, F = 5 at L = 1, 3, 9 (level blocks of 1, 4 and 8), F = 32 at L = 1.
Every output was recorded twice on the parent in one process and was the same both times.
The four fp32_kernel cases of item 4 (mean_fp32_F5_L2, mean_fp32_F14_L2, mean_fp32_F5_L17, mean_fp32_F14_L17) are NOT the parent's
bits any more: the mixed-precision mode now centres every feature column and T on its first element in fp64 before the fp32
rounding (centred_value, gpslc_internal.h), which changes its results by design.  Their entries (the fixture's
"fp32_entries" note names them) are the bits of the commit that introduced the centring, recorded twice in one process on an
MI355X like the others; all other entries passed unchanged on that commit.  They stay bit-for-bit assertions.
The work replaced: src/estimation.jl:36-163, src/likelihood.jl:8-174."""
import hashlib
import json
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_build_parent_hashes.json")
FEAT = {0: ("T", 0, 0), 1: ("U", 1, 0), 3: ("UX", 1, 2), 5: ("UX", 2, 3), 6: ("UX", 2, 4), 7: ("UX", 2, 5), 9: ("UX", 3, 6),
        11: ("UX", 3, 8), 14: ("UX", 5, 9), 18: ("UX", 6, 12), 32: ("UX", 8, 24)}     # F -> (shape, nU, nX)
LD_BLOCKS = ("CovWW", "CovWWs", "CovWWp", "CovC11", "CovC12", "CovC21", "CovC22")
OUTPUTS = {"ite": ("MeanITEs", "CovITEs"), "ld": LD_BLOCKS, "draws": ("meanSATE", "varSATE", "MeanITE", "draws"),
           "mean": ("meanSATE", "varSATE", "MeanITE"), "vec": ("meanSATE", "varSATE", "MeanITE")}


def _digest(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return hashlib.sha256(repr(x.shape).encode() + x.tobytes()).hexdigest()


def _case(n, F, seed):
    shape, nU, nX = FEAT[F]
    return cases.make_case(n, shape, False, S=2, nU=max(nU, 1), nX=max(nX, 1), seed=seed)


def _vector(n, seed, L=None):
    rng = np.random.Generator(np.random.Philox(9000 + seed))
    return rng.uniform(-1.0, 1.0, n if L is None else (L, n))


def _ite(gp, n, F, form, seed):
    c = _case(n, F, seed)
    g = cases.gpslc_object(gp, c)
    if form == "plain":
        out = gp.ITEDistributions(g, float(c["T"][n // 3]))        # row n // 3 of D is the exact-zero row rule's
    elif form == "vector":
        out = gp.ITEDistributions(g, _vector(n, seed))
    elif form == "vector_eq_T":
        out = gp.ITEDistributions(g, c["T"].copy())
    elif form == "contrast":
        out = gp.ITEDistributions(g, 0.6, baseline=-0.3)
    else:
        assert form == "contrast_a_eq_b"
        out = gp.ITEDistributions(g, 0.6, baseline=0.6)
    g.ctx().close()
    return out


def _ld(gp, n, F, form, seed):
    c = _case(n, F, seed)
    p = cases.samples_of(c)[1]
    doT = 0.4 if form == "scalar" else _vector(n, seed)
    return gp.likelihoodDistribution(p.uyLS, p.xyLS, p.tyLS, p.yNoise, p.yScale, p.U, c["X"], c["T"], c["Y"], doT)[1:]


def _draws(gp, n, F, form, seed):
    c = _case(n, F, seed)
    g = cases.gpslc_object(gp, c)
    L = 3
    levels = _vector(n, seed, L) if form == "vector" else np.linspace(-0.6, 0.8, L)
    base = np.linspace(0.5, -0.5, L) if form == "contrast" else None
    out = gp.predict(g, levels, baseline=base, want_mean_ite=True, spp=2, seed=11, want_draws=True)
    g.ctx().close()
    return out


def _mean(gp, n, F, form, L, seed):
    c = _case(n, F, seed)
    g = cases.gpslc_object(gp, c, fp32_kernel=(form == "fp32"))
    levels = np.linspace(-0.6, 0.8, L) if L > 1 else np.array([0.4])
    base = np.linspace(0.5, -0.5, L) if form == "contrast" else None
    out = gp.predict(g, levels, baseline=base, want_mean_ite=True)
    g.ctx().close()
    return out


def _vec(gp, n, F, L, seed):
    c = _case(n, F, seed)
    g = cases.gpslc_object(gp, c)
    out = gp.predict(g, _vector(n, seed, L), want_mean_ite=True)
    g.ctx().close()
    return out


RUN = {"ite": _ite, "ld": _ld, "draws": _draws, "mean": _mean, "vec": _vec}
CASES = {}
for _i, _form in enumerate(("plain", "vector", "contrast")):
    for _j, (_n, _F) in enumerate(((128, 5), (129, 5), (200, 5), (129, 0), (129, 1), (129, 7), (129, 32))):
        CASES[f"ite_{_form}_n{_n}_F{_F}"] = ("ite", _n, _F, _form, 400 + 10 * _i + _j)
CASES["ite_vector_eq_T_n129_F5"] = ("ite", 129, 5, "vector_eq_T", 430)
CASES["ite_contrast_a_eq_b_n129_F5"] = ("ite", 129, 5, "contrast_a_eq_b", 431)
for _i, _form in enumerate(("scalar", "vector")):
    for _j, (_n, _F) in enumerate(((128, 5), (129, 5), (200, 5), (129, 0), (129, 32))):
        CASES[f"ld_{_form}_n{_n}_F{_F}"] = ("ld", _n, _F, _form, 440 + 10 * _i + _j)
for _i, _form in enumerate(("plain", "vector", "contrast")):
    CASES[f"draws_{_form}_n129_L3"] = ("draws", 129, 5, _form, 460 + _i)
for _i, _L in enumerate((1, 2)):
    for _j, _F in enumerate((3, 5, 6, 7, 9, 11, 14, 18, 32)):
        CASES[f"mean_fp64_F{_F}_L{_L}"] = ("mean", 200, _F, "plain", _L, 470 + 10 * _i + _j)
CASES["mean_contrast_F5_L2"] = ("mean", 200, 5, "contrast", 2, 490)
for _i, _L in enumerate((2, 17)):
    for _j, _F in enumerate((5, 14)):
        CASES[f"mean_fp32_F{_F}_L{_L}"] = ("mean", 200, _F, "fp32", _L, 491 + 2 * _i + _j)
for _i, (_F, _L) in enumerate(((5, 1), (5, 3), (5, 9), (32, 1))):
    CASES[f"vec_F{_F}_L{_L}"] = ("vec", 129, _F, _L, 500 + _i)


def case_ids():
    return list(CASES)


def compute(gp, case_id):
    kind, *args = CASES[case_id]
    return {k: _digest(a) for k, a in zip(OUTPUTS[kind], RUN[kind](gp, *args))}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case_id", case_ids())
def test_outputs_equal_the_parents_bit_for_bit(gp, recorded, case_id):
    """Bit for bit against the fixture: the parent's bits, except the four mean_fp32_* cases, which hold the bits of the commit
    that centred the fp32 mode's features (module docstring)."""
    assert compute(gp, case_id) == recorded["hashes"][case_id], case_id


def test_every_case_was_recorded_and_was_repeatable_on_the_parent(recorded):
    """The fixture itself: every case is there, with every output, and the parent's second run gave the first one's bits."""
    assert len(case_ids()) == 63
    assert sorted(recorded["hashes"]) == sorted(case_ids())
    assert len(recorded["parent"]) == 40
    assert recorded["hashes"] == recorded["second_run"]
    for cid in case_ids():
        assert sorted(recorded["hashes"][cid]) == sorted(OUTPUTS[CASES[cid][0]]), cid
