"""The full ITE covariance and the predictive draws (gpslc_predict's unit B and C: ITEDistributions, sampleITE,
predictCounterfactualEffects) against the host reference of tests/batched_reference.py, at the shapes where the draw path
changes hands:

- odd tile counts (nt = 3, 5, 7: the streaming draw kernel pairs tile rows (nt-1-p, p) and leaves the middle row alone) and
  ragged last tiles, both parities of n;
- every draw kernel (spp <= 16, the 2 / 4 / 8 block variants, a second pass of the stream kernel beyond 128) at odd nt;
- the library's Philox normals at size (odd n: the element-wise branch of the operand staging; spp > 128: the staging of a second pass);
- sub-batches of (sample, level) pairs beyond the first: sample groups at g0 > 0, level chunks at l0 > 0, the 32-level chunks
  of the level-sweep scatter, a gpslc_set_ensemble placement, and the chunking of gpslc_set_tuning (bit for bit);
- the documented example's call (NEEC: 91 samples x 101 levels x 2 draws, jitter 1e-10);
- the CovITE failure codes of gpslc_last_info / PosDefException: n + the pivot of the sample's lowest-index failing level.

Unless a test says otherwise the jitter is predictionCovarianceNoise = 1e-3: cond(CovITE) stays small, so every draw column
is held to cases.draw_bounds' tight bound."""
import numpy as np
import pytest

import batched_reference as br
import cases
import gpslc_oracle as orc
import vector_restatement as vr

pytestmark = pytest.mark.gpu

PN = 1e-3
PROF_DRAWS = 2           # profile class of the draw launches (unit C)


def _obj(gp, c, pn=PN, profile=False, max_batch=0, n_streams=0):
    g = cases.gpslc_object(gp, c, hyperparams=gp.HyperParameters(predictionCovarianceNoise=pn))
    if profile or max_batch or n_streams:
        g._ctx = gp.Context(g.getN(), g.getNX(), g.getNU(), profile=profile)
        g._ctx.set_data(g.X, g.T, g.Y)
        if max_batch or n_streams:
            g._ctx.set_tuning(max_batch, 0, n_streams)
    return g


def _philox_z(seed, n, spp, S, L, s_off=0, S_total=0):
    """the library's normals as predict's z (n, spp, S, L): stream (s + s_off) + S_total * l (S_total = 0: the call's S)"""
    St = S_total or S
    z = np.zeros((n, spp, S, L))
    for s in range(S):
        for l in range(L):
            z[:, :, s, l] = orc.philox_normals(seed, s + s_off + St * l, n * spp).reshape(n, spp, order="F")
    return z


def _check_draws(dr, c, doTs, pairs, z, pn=PN, tight=True):
    """dr (L, n, S*spp) of gpslc_predict against M + chol(CovITE + pn I) z for the listed (s, l) pairs; z (n, spp, S, L)"""
    spp = z.shape[1]
    zp = np.stack([z[:, :, s, l] for s, l in pairs])
    ref = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, pairs, doTs, zp, pn)
    for j, (s, l) in enumerate(pairs):
        got = dr[l][:, s * spp:(s + 1) * spp]
        ok, worst = br.draws_match(got, ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j], zp[j], tight=tight)
        assert ok, (s, l, worst, ref["lam_max"][j] / ref["lam_min"][j])
    return ref


def _all_pairs(S, L):
    return [(s, l) for s in range(S) for l in range(L)]


def _check_ite_distributions(gp, g, c, doT, pn=PN):
    """ITEDistributions (MeanITEs S x n, CovITEs S x n x n) against ite_pairs: M at 1e-9 relative, every CovITE entry at 1e-10 of
    max |C|, C exactly symmetric; doT a scalar or an (n,) vector"""
    S = c["S"]
    M, Cv = gp.ITEDistributions(g, doT)
    d = np.asarray(doT, dtype=np.float64)
    levels = d[None] if d.ndim == 1 else np.array([float(d)])
    ref = br.ite_pairs(c["X"], c["T"], c["Y"], c, [(s, 0) for s in range(S)], levels, pn)
    for s in range(S):
        assert np.max(np.abs(M[s] - ref["mean"][s])) <= 1e-9 * np.max(np.abs(ref["mean"][s])), s
        assert np.max(np.abs(Cv[s] - ref["cov"][s])) <= 1e-10 * np.max(np.abs(ref["cov"][s])), s
        assert np.array_equal(Cv[s], Cv[s].T), s


# ---- tile counts -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [255, 257, 383, 384, 385, 513, 639, 770, 895])
def test_draws_at_every_tile_count(gp, n):
    """nt = 2 .. 7 with full and ragged last tiles, L = 1 (the reference tensor written directly) and L = 3 (staging + scatter);
    every pair, every draw.  At n in {257, 639, 895} also ITEDistributions, scalar and per-individual level."""
    S, spp = 2, 10
    c = cases.make_case(n, "UX", False, S=S, seed=n)
    g = _obj(gp, c)
    for L in (1, 3):
        doTs = np.linspace(-0.7, 0.9, L)
        z = np.random.default_rng(n + L).standard_normal((n, spp, S, L))
        _, _, _, dr = gp.predict(g, doTs, spp=spp, z=z, want_draws=True)
        assert dr.shape == (L, n, S * spp)
        _check_draws(dr, c, doTs, _all_pairs(S, L), z)
        assert not g.ctx().last_info(S).any()
    if n in (257, 639, 895):
        _check_ite_distributions(gp, g, c, 0.35)
        _check_ite_distributions(gp, g, c, vr.policy(c, 2, seed=n)[1])


# ---- every draw kernel at an odd tile count ------------------------------------------------------------------------------

SPPS = (1, 16, 17, 32, 33, 64, 65, 128, 129, 130)


@pytest.mark.parametrize("n", [639, 384])
def test_every_draw_kernel_at_an_odd_tile_count(gp, n):
    """spp across the draw kernels (<= 16, <= 32, <= 64, <= 128: the streaming kernel's block variants; > 128: a second pass
    of one or two draws) at nt = 5 (ragged) and nt = 3 (full tiles), L = 1, every draw.  One host factor per pair
    serves every spp (the reference draws with all columns of z at once)."""
    S = 2
    c = cases.make_case(n, "UX", False, S=S, seed=3 * n)
    doTs = np.array([0.25])
    z_all = np.random.default_rng(n).standard_normal((n, sum(SPPS), S, 1))
    g = _obj(gp, c, profile=True)
    outs = []
    for spp in SPPS:
        o = sum(SPPS[:SPPS.index(spp)])
        z = np.asfortranarray(z_all[:, o:o + spp])
        g.ctx().profile_reset()
        _, _, _, dr = gp.predict(g, doTs, spp=spp, z=z, want_draws=True)
        assert g.ctx().profile_get(PROF_DRAWS)[0] > 0, spp
        outs.append(dr)
    zp = np.stack([z_all[:, :, s, 0] for s in range(S)])
    ref = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, [(s, 0) for s in range(S)], doTs, zp, PN)
    for spp, dr in zip(SPPS, outs):
        o = sum(SPPS[:SPPS.index(spp)])
        for s in range(S):
            ok, worst = br.draws_match(dr[0][:, s * spp:(s + 1) * spp], ref["draws"][s][:, o:o + spp],
                                       ref["lam_min"][s], ref["lam_max"][s], zp[s][:, o:o + spp])
            assert ok, (spp, s, worst)


# ---- Philox normals at size ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [383, 770])
@pytest.mark.parametrize("spp", [10, 130])
def test_philox_draws_at_size(gp, n, spp):
    """Seeded draws = the same call with z from orc.philox_normals(seed, s + S*l, n*spp) (1e-12 of max |draw|: host and device
    libm may differ by an ulp) and = the host reference; odd and even n, the staged image of one pass (spp <= 128) and of two."""
    S, L, seed = 2, 2, 20 + n + spp
    c = cases.make_case(n, "UX", False, S=S, seed=n + spp)
    doTs = np.array([-0.2, 0.5])
    g = _obj(gp, c)
    _, _, _, dr_p = gp.predict(g, doTs, spp=spp, seed=seed, want_draws=True)
    z = _philox_z(seed, n, spp, S, L)
    _, _, _, dr_z = gp.predict(g, doTs, spp=spp, z=z, want_draws=True)
    assert np.max(np.abs(dr_p - dr_z)) <= 1e-12 * np.max(np.abs(dr_z))
    _check_draws(dr_p, c, doTs, _all_pairs(S, L), z)


# ---- draws per unit do not change a draw ---------------------------------------------------------------------------------

SPP_PAIRS = ((128, 130), (128, 257), (130, 257))


@pytest.mark.parametrize("n", [129, 256, 383])
def test_draw_bits_do_not_depend_on_spp(gp, n):
    """The same case and seed with spp = 128, 130 and 257 draws per unit (one pass over the factor, a second pass of two draws,
    two full passes and one draw): column s*spp + d of a shorter call equals column s*spp' + d of a longer one BIT FOR BIT,
    for every d both have — seeded (element e = g + n d and the Philox stream do not depend on spp) and with the caller's z
    (the shorter call's z is the longer call's leading draw columns): a draw's column depends only on its z column and on
    the factor.  n = 129: odd, one live row in tile 2; 256: even, two full tiles (the pair branch of the staging);
    383: nt = 3, the middle tile row has no partner."""
    S, seed = 2, 900 + n
    c = cases.make_case(n, "UX", False, S=S, seed=n)
    g = _obj(gp, c)
    doTs = np.array([0.3])
    z_all = np.random.default_rng(n).standard_normal((n, 257, S, 1))
    seeded, given = {}, {}
    for spp in (128, 130, 257):
        seeded[spp] = gp.predict(g, doTs, spp=spp, seed=seed, want_draws=True)[3]
        given[spp] = gp.predict(g, doTs, spp=spp, z=np.asfortranarray(z_all[:, :spp]), want_draws=True)[3]
        assert seeded[spp].shape == (1, n, S * spp)
    for form, dr in (("seeded", seeded), ("z", given)):
        for a, b in SPP_PAIRS:
            for s in range(S):
                assert np.array_equal(dr[a][0][:, s * a:(s + 1) * a], dr[b][0][:, s * b:s * b + a]), (form, n, a, b, s)


# ---- sub-batch splits at nt >= 3 -----------------------------------------------------------------------------------------

N_SPLIT = 383            # nt = 3, ragged last tile; the sub-batch holds Bb = 128 pairs
SPLITS = {               # (S, L): what the sub-batches of one chunk are
    "sample_groups": (3, 50),      # gs_max = 2: the second sample group at g0 = 2
    "level_chunks": (2, 130),      # lc_max = 128: a level chunk at l0 = 128 with lc = 2; the scatter's 32-level chunks
    "one_level": (130, 1),         # gs_max = 128: a sample group at g0 = 128
}
ENS = (5, 140)           # gpslc_set_ensemble(s_off, S_total) of the seeded repeats


def _split_case(name):
    S, L = SPLITS[name]
    c = cases.make_case(N_SPLIT, "UX", False, S=S, seed=len(name) + S)
    doTs = np.linspace(-0.9, 1.2, L)
    return c, doTs


@pytest.fixture(scope="module")
def split_runs(gp):
    """Each split case once with the caller's normals (the Philox stream of the ENS placement) and once seeded under it."""
    out = {}
    for name in SPLITS:
        c, doTs = _split_case(name)
        S, L = SPLITS[name]
        spp, seed = 2, 77
        z = _philox_z(seed, N_SPLIT, spp, S, L, *ENS)
        g = _obj(gp, c)
        _, _, _, dr = gp.predict(g, doTs, spp=spp, z=z, want_draws=True)
        g.ctx().set_ensemble(*ENS)
        _, _, _, dr_p = gp.predict(g, doTs, spp=spp, seed=seed, want_draws=True)
        g.ctx().set_ensemble(0, 0)
        out[name] = dict(c=c, doTs=doTs, z=z, dr=dr, dr_p=dr_p, spp=spp, seed=seed)
    return out


@pytest.mark.parametrize("name", list(SPLITS))
def test_draws_in_later_sub_batches(gp, split_runs, name):
    """Every pair of every sub-batch against the host reference; the seeded repeat under gpslc_set_ensemble(5, 140) draws
    the oracle stream s + 5 + 140 l."""
    r = split_runs[name]
    S, L = SPLITS[name]
    assert r["dr"].shape == (L, N_SPLIT, S * r["spp"])
    _check_draws(r["dr"], r["c"], r["doTs"], _all_pairs(S, L), r["z"])
    assert np.max(np.abs(r["dr_p"] - r["dr"])) <= 1e-12 * np.max(np.abs(r["dr"]))


def test_ite_distributions_in_a_later_sample_group(gp, split_runs):
    """S = 130 at one level: gather_cov_kernel writes the sample group at g0 = 128."""
    r = split_runs["one_level"]
    g = _obj(gp, r["c"])
    _check_ite_distributions(gp, g, r["c"], float(r["doTs"][0]))


@pytest.mark.parametrize("name,k", [("sample_groups", 1), ("sample_groups", 2), ("sample_groups", 7),
                                    ("one_level", 1), ("one_level", 2), ("one_level", 7), ("one_level", 129)])
def test_chunking_does_not_change_the_draws(gp, split_runs, name, k):
    """gpslc_set_tuning(max_batch = k, n_streams = 2): chunks at s0 > 0 on alternating streams, each with its own sub-batches
    (k = 129 at S = 130: a chunk with a sample group at g0 = 128, then a chunk at s0 = 129) — bit-identical to the default."""
    r = split_runs[name]
    g = _obj(gp, r["c"], max_batch=k, n_streams=2)
    _, _, _, dr = gp.predict(g, r["doTs"], spp=r["spp"], z=r["z"], want_draws=True)
    assert np.array_equal(dr, r["dr"])


def test_chunks_with_later_sample_groups_do_not_change_the_draws(gp):
    """S = 6, L = 50, max_batch = 3: the second chunk (s0 = 3) has its own second sample group (g0 = 2) — bit-identical to the
    default call, and the second chunk's pairs against the host reference."""
    S, L, spp = 6, 50, 2
    c = cases.make_case(N_SPLIT, "UX", False, S=S, seed=66)
    doTs = np.linspace(-0.5, 0.8, L)
    z = np.random.default_rng(6).standard_normal((N_SPLIT, spp, S, L))
    _, _, _, dr = gp.predict(_obj(gp, c), doTs, spp=spp, z=z, want_draws=True)
    _, _, _, dr3 = gp.predict(_obj(gp, c, max_batch=3, n_streams=2), doTs, spp=spp, z=z, want_draws=True)
    assert np.array_equal(dr3, dr)
    _check_draws(dr, c, doTs, [(s, l) for s in (3, 5) for l in (0, 31, 32, 49)], z)


# ---- the documented workload ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def neec_chain(gp):
    """docs/example_data/NEEC_Example.jl:7-30: gpslc(nOuter = 100, nU = 2, nMHInner = 3, nESInner = 5) on the NEEC sample"""
    import os
    hp = gp.getHyperParameters()
    hp.nOuter, hp.nU, hp.nMHInner, hp.nESInner = 100, 2, 3, 5
    g = gp.gpslc(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neec", "NEEC_sampled.csv"),
                 hyperparams=hp, seed=1234)
    assert gp.getNumPosteriorSamples(g) == 91
    return g


def test_documented_example_draws_match_the_reference(gp, neec_chain):
    """predictCounterfactualEffects(g, 2, fidelity = 100, seed = 3) at the default jitter 1e-10: every level of samples 0, 45
    and 90 against M + chol(CovITE + 1e-10 I) z with z from the Philox stream s + 91 l, within draw_bounds' conditioning-aware
    bound; every other draw finite, every failure code 0."""
    g = neec_chain
    spp, seed = 2, 3
    ite, doT = gp.predictCounterfactualEffects(g, spp, fidelity=100, seed=seed)
    n, S, L = g.getN(), g.getNumPosteriorSamples(), len(doT)
    assert ite.shape == (L, n, S * spp) and L == 101
    assert np.all(np.isfinite(ite))
    assert not g.ctx().last_info(S).any()
    post = dict(U=g.U, uyLS=g.uyLS, xyLS=g.xyLS, tyLS=g.tyLS, yNoise=g.yNoise, yScale=g.yScale)
    c = dict(post, X=g.X, T=g.T, Y=g.Y, S=S)
    pairs = [(s, l) for s in (0, 45, 90) for l in range(L)]
    zp = np.stack([orc.philox_normals(seed, s + S * l, n * spp).reshape(n, spp, order="F") for s, l in pairs])
    ref = br.ite_pair_draws(c["X"], c["T"], c["Y"], c, pairs, doT, zp, g.hyperparams.predictionCovarianceNoise)
    for j, (s, l) in enumerate(pairs):
        ok, worst = br.draws_match(ite[l][:, s * spp:(s + 1) * spp], ref["draws"][j], ref["lam_min"][j], ref["lam_max"][j],
                                   zp[j], tight=False)
        assert ok, (s, l, worst)


# ---- CovITE failure codes ------------------------------------------------------------------------------------------------
# A case whose CovITE + pred_noise I (pred_noise < 0) fails at a chosen pivot, unambiguously: B nearly diagonal (individuals
# far apart in X), treatments far from every level except one "near" individual per failing level (T = doT + 0.01).  At the
# near individual CovITE's diagonal is ~2 yScale (1 - r), tiny for a long tyLS and ~0.08 for a short one; everywhere else it
# is O(yScale).  So with a shift of -1e-3 a sample with tyLS = 3 fails exactly at the near individual, one with tyLS = 0.05
# never.  The host checks the margins before anything runs on the GPU.

N_FAIL = 383
SHIFT = -1e-3
TYLS = (0.05, 3.0, 0.05)         # sample 1 fails


def _fail_case(L, near):
    """near: {level: 0-based individual}; levels 0.3 l"""
    n, S = N_FAIL, len(TYLS)
    rng = np.random.default_rng(L + len(near))
    doTs = 0.3 * np.arange(L)
    T = -20.0 - rng.random(n)
    for l, i in near.items():
        T[i] = doTs[l] + 0.01
    X = np.arange(n, dtype=np.float64)[:, None]
    Y = np.sin(T) + 0.1 * rng.standard_normal(n)
    c = dict(n=n, S=S, X=X, T=T, Y=Y, U=None, uyLS=None, xyLS=np.full((1, S), 0.3), tyLS=np.array(TYLS),
             yNoise=np.full(S, 0.1), yScale=np.ones(S))
    return c, doTs


def _expected_codes(c, doTs, levels):
    """per sample: n + the first failing pivot of its lowest-index failing level among `levels` (0 = none); asserts that each
    failing pivot is unambiguous (pivot <= -1e-6 max diag, every earlier one >= +1e-6 max diag) and that non-failing
    factors keep the same margin"""
    n, S = c["n"], c["S"]
    want = np.zeros(S, dtype=np.int64)
    pairs = [(s, l) for s in range(S) for l in levels]
    ref = br.ite_pairs(c["X"], c["T"], c["Y"], c, pairs, doTs, SHIFT)
    for j, (s, l) in enumerate(pairs):
        C = ref["cov"][j]
        tol = 1e-6 * np.max(np.diag(C))
        p = br.first_failing_pivot(C)
        if p == 0:
            assert np.min(np.diag(np.linalg.cholesky(C))) ** 2 >= tol, (s, l)
            continue
        earlier, d = br.schur_pivots(C, p)
        assert d <= -tol and (earlier.size == 0 or earlier.min() >= tol), (s, l, p, d)
        if want[s] == 0:
            want[s] = n + p
    return want


@pytest.mark.parametrize("pivot", [41, 128, 129, 371])
def test_covite_failure_code_names_the_pivot(gp, pivot):
    """In the first tile, on both sides of the first tile boundary and in the ragged last tile: last_info = n + pivot for the
    failing sample, 0 for the others; PosDefException.info the first nonzero code in sample order."""
    c, doTs = _fail_case(1, {0: pivot - 1})
    want = _expected_codes(c, doTs, [0])
    assert list(want) == [0, N_FAIL + pivot, 0]
    g = _obj(gp, c, pn=SHIFT)
    z = np.random.default_rng(pivot).standard_normal((N_FAIL, 1, c["S"], 1))
    with pytest.raises(gp.PosDefException) as e:
        gp.predict(g, doTs, spp=1, z=z, want_draws=True)
    assert e.value.info == N_FAIL + pivot
    assert list(g.ctx().last_info(c["S"])) == list(want)


# the failing levels of sample 1: {level: 0-based individual}.  Inside one sub-batch the lowest-index failing level (1)
# breaks down in a later tile column than level 2; across the level-chunk boundary of L = 130, level 100 (first chunk) in a
# later one than level 129 (second chunk)
MULTI = {"one_sub_batch": (3, {1: 300, 2: 10}), "across_level_chunks": (130, {100: 300, 129: 10})}


@pytest.mark.parametrize("name", list(MULTI))
def test_covite_failure_code_is_the_lowest_failing_level(gp, name):
    """A sample whose levels fail at different pivots reports the pivot of its lowest-index failing level — the level the
    reference's loop (src/prediction.jl:30-33) reaches first — on every repeat and under every gpslc_set_tuning."""
    L, near = MULTI[name]
    c, doTs = _fail_case(L, near)
    want = _expected_codes(c, doTs, sorted(near) + [0])
    assert list(want) == [0, N_FAIL + 301, 0]
    z = np.random.default_rng(L).standard_normal((N_FAIL, 1, c["S"], L))
    g = _obj(gp, c, pn=SHIFT)
    for tuning in (None, None, (1, 2), (2, 2)):
        if tuning is not None:
            g = _obj(gp, c, pn=SHIFT, max_batch=tuning[0], n_streams=tuning[1])
        with pytest.raises(gp.PosDefException) as e:
            gp.predict(g, doTs, spp=1, z=z, want_draws=True)
        assert e.value.info == N_FAIL + 301, tuning
        assert list(g.ctx().last_info(c["S"])) == list(want), tuning
