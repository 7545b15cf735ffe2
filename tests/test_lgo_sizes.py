"""The group sizes and placements of tests/test_gpu_lgo_sizes.py without a GPU: the labellings are what they claim to be —
sizes, padded sizes, the tile row of every group's first member (the kernel's k0) and the tile rows its members span — and the
restatement's two computations agree on them far inside the bound the device is held to (at most 1e-3 of
max(1e-10, 1e-14 cond(A) max_g cond(C_g))), so that what the GPU test measures is the device."""
import functools

import numpy as np
import pytest

import cases
import lgo_restatement as lg


@functools.lru_cache(maxsize=None)
def _case(n, seed):
    return cases.make_case(n, "UX", False, S=2, seed=seed)


LAB = lg.size_labellings()


def test_the_labellings_are_what_they_claim():
    sizes = {k: np.bincount(v).tolist() for k, v in LAB.items()}
    rows = {k: lg.tile_rows(v) for k, v in LAB.items()}
    assert all(v.shape == (640,) and v.dtype == np.int32 for v in LAB.values())
    assert sizes["contiguous"] == list(lg.SIZES) == sizes["scattered"] and sum(lg.SIZES) == 640
    assert [r[0] for r in rows["contiguous"]] == [0, 0, 0, 1, 1, 2, 3, 3, 4]
    assert [len(r) for r in rows["contiguous"]] == [1, 1, 2, 1, 2, 2, 1, 2, 1]             # which ones straddle a boundary
    assert all(r == [0, 1, 2, 3, 4] for r in rows["scattered"])
    assert not np.array_equal(LAB["scattered"], LAB["contiguous"])
    assert sizes["late"] == [17] * 15 + [1] + list(lg.LATE_SIZES)
    assert all(r == [2, 3, 4] for r in rows["late"][16:]) and all(r[-1] <= 1 for r in rows["late"][:16])
    assert sizes["later"] == [17] * 7 + [9] + list(lg.LATER_SIZES)
    assert all(r[0] == 1 and len(r) >= 3 for r in rows["later"][8:]) and all(r == [0] for r in rows["later"][:8])
    # every layout of the kernel with k0 > 0 and members in three tile rows or more
    late = {lg.padded(m) for name, skip in (("late", 16), ("later", 8)) for m in sizes[name][skip:]}
    assert late == set(range(16, 129, 16))
    # the layouts the older labellings never reach, on one tile row, across a boundary and over all five
    assert {48, 80, 96} <= {lg.padded(m) for m in lg.SIZES}


@pytest.mark.parametrize("name", sorted(LAB))
def test_the_hosts_own_error_is_far_inside_the_bound(name):
    c = _case(640, 700)
    exp = lg.expected(c, LAB[name])
    for s, e in exp.items():
        errs = lg.errors(e["closed"], e["refit"], e["q"], c["Y"], LAB[name])
        print(name, "sample", s, "cond(A) %.3g cond(C) %.3g tol %.3g" % (e["cond"], e["cond_c"], e["tol"]), "host (var, mean, lpd)", errs)
        assert max(errs) <= 1e-3 * e["tol"], errs


def test_the_size_edges_are_scattered_over_every_tile_row():
    assert [lg.padded(m) for m in (15, 16, 17, 128)] == [16, 16, 32, 128]
    assert {lg.padded(m) for m in lg.EDGE_SIZES} == set(range(16, 129, 16))
    for m in lg.EDGE_SIZES:
        I = lg.edge_group(m)
        assert I.shape == (m,) and len(set(I.tolist())) == m and np.all(np.diff(I) > 0) and I[-1] < lg.EDGE_N
        assert sorted(set((I // 128).tolist())) == [0, 1, 2]
        assert np.array_equal(I, np.sort(np.intersect1d(I, lg.edge_group(128))))          # nested: one permutation
        for rest in (17, 1):
            lab = lg.beside(lg.EDGE_N, I, rest)
            sizes = np.bincount(lab)
            assert lab.dtype == np.int32 and sizes[0] == m and np.array_equal(np.flatnonzero(lab == 0), I)
            assert sizes.min() >= 1 and sizes[1:].max() == rest and sizes.sum() == lg.EDGE_N


@pytest.mark.parametrize("m", lg.EDGE_SIZES)
def test_the_hosts_own_error_on_the_size_edges(m):
    c = _case(lg.EDGE_N, 701)
    lab = lg.beside(lg.EDGE_N, lg.edge_group(m), 17)
    e = lg.expected(c, lab, samples=(0,))[0]
    errs = lg.errors(e["closed"], e["refit"], e["q"], c["Y"], lab)
    print("m", m, "cond(A) %.3g cond(C) %.3g tol %.3g" % (e["cond"], e["cond_c"], e["tol"]), "host (var, mean, lpd)", errs)
    assert max(errs) <= 1e-3 * e["tol"], errs
