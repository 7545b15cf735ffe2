"""Leave-group-out checks on the GPU over group sizes and placements (gpslc_y_lgo).  lgo_group_kernel picks its
layout from the padded group size mp = 16 ceil(m / 16) — slab width KC = 128, 64, 32, 32, 16, 16, 16, 16, elements per thread
KC mp / 256 = 8, 8, 6, 8, 5, 6, 7, 8 and 1, 3, 6, 10, 15, 21, 28, 36 lower blocks of C over four waves for mp = 16 .. 128 — and
starts its gather at the tile row k0 of the group's first member.  tests/test_gpu_lgo.py reaches mp = 16, 32, 64, 112, 128 and
k0 > 0 only for small groups; here (labellings in tests/lgo_restatement.py, pinned by tests/test_lgo_sizes.py on the CPU):

  five tiles, groups of 33 .. 112 contiguous, scattered over all tile rows, and starting late (k0 = 1 and 2) at every mp;
  every size around a multiple of 16 from 15 to 128 as one group scattered over three tiles, beside blocks of 17 and beside
  singletons (another launch, another largest group: the same bits);
  groups of one launch against the same groups beside singletons only; an fp32-kernel context.

Bound: test_gpu_lgo._check with lg.expected / lg.errors / lg.tolerance unchanged — max(1e-10, 1e-14 cond(A) max_g cond(C_g)), the
closed form against the literal refit first, then the device against the refit."""
import functools

import numpy as np
import pytest

import cases
import lgo_restatement as lg
from test_gpu_lgo import _call, _check

pytestmark = pytest.mark.gpu
LAB = lg.size_labellings()


@functools.lru_cache(maxsize=None)
def _case(n, seed):
    return cases.make_case(n, "UX", False, S=2, seed=seed)


@functools.lru_cache(maxsize=None)
def _object(gp, n, seed, **kw):
    return cases.gpslc_object(gp, _case(n, seed), **kw)


@functools.lru_cache(maxsize=None)
def _expected(name):
    return lg.expected(_case(lg.SIZES_N, 700), LAB[name])


@functools.lru_cache(maxsize=None)
def _device(gp, name):
    return _call(gp, _object(gp, lg.SIZES_N, 700), LAB[name])


# ---- 1. every layout, across tile rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAB))
def test_every_layout_across_tile_rows(gp, name):
    c, labels = _case(lg.SIZES_N, 700), LAB[name]
    got = _device(gp, name)
    G = int(labels.max()) + 1
    assert got[0].shape == (640, 2) and got[1].shape == (640, 2) and got[2].shape == (G, 2)
    assert all(np.all(np.isfinite(a)) for a in got)
    _check(_expected(name), got, c["Y"], labels, what=name)
    assert not _object(gp, lg.SIZES_N, 700).ctx().last_info(2).any()


# ---- 2. size edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", lg.EDGE_SIZES)
def test_size_edges(gp, m):
    """one group of m members scattered over three tiles beside blocks of 17, against the refit; then beside singletons: the
    group's rows of lgoMean and lgoVar and its lgoLpd are the same bits (nothing depends on the other groups —
    nor on the launch's LDS size, which is the largest group's)"""
    n = lg.EDGE_N
    c, g = _case(n, 701), _object(gp, n, 701)
    I = lg.edge_group(m)
    a, b = lg.beside(n, I, 17), lg.beside(n, I, 1)
    got = _call(gp, g, a)
    _check(lg.expected(c, a, samples=(0,)), got, c["Y"], a, what=f"m={m}")
    alone = _call(gp, g, b)
    assert np.all(np.isfinite(got[0][I])) and np.all(got[1][I] > 0.0)
    assert np.array_equal(alone[0][I], got[0][I]) and np.array_equal(alone[1][I], got[1][I])
    assert np.array_equal(alone[2][0], got[2][0])


# ---- 3. one launch for groups of every size against each group on its own -------------------------------------------------------
@pytest.mark.parametrize("size", [33, 80, 112])
def test_a_group_of_a_mixed_launch_beside_singletons(gp, size):
    labels = LAB["scattered"]
    k = lg.SIZES.index(size)
    I = np.flatnonzero(labels == k)
    assert len(I) == size
    mixed = _device(gp, "scattered")
    alone = _call(gp, _object(gp, lg.SIZES_N, 700), lg.beside(lg.SIZES_N, I, 1))
    assert np.array_equal(alone[0][I], mixed[0][I]) and np.array_equal(alone[1][I], mixed[1][I])
    assert np.array_equal(alone[2][0], mixed[2][k])


# ---- 4. an fp32-kernel context ----------------------------------------------------------------------------------------------
def test_fp32_context_on_the_contiguous_labelling(gp):
    """the bound of test_gpu_lgo.test_fp32_context_against_the_fp64_restatement: 1e-6"""
    c, labels = _case(lg.SIZES_N, 700), LAB["contiguous"]
    g = cases.gpslc_object(gp, c, fp32_kernel=True)
    _check(_expected("contiguous"), _call(gp, g, labels), c["Y"], labels, tol=1e-6, what="fp32 contiguous")
    g.ctx().close()
