"""K-fold cross-validation without a GPU (gpslc_y_kfold, `kfoldPredictive`): the labellings of
tests/test_gpu_kfold.py pinned — group sizes, tile counts of the large groups, the tile rows their chains start at — with the
host restatement's two computations agreeing on them a thousand times inside the bound the device is held to; and the Python
front end through the recorder seam of tests/test_frontend_dispatch.py."""
import ctypes
import os

import numpy as np
import pytest

import cases
import kfold_cases as kc
import lgo_restatement as lg
from test_frontend_dispatch import _array, recording

# name -> (sizes of the groups beyond 128 members, their tile counts, the first tile row of every row block's chain per large
# group in label order, number of groups of at most 128 members)
PINNED = {
    300: {"everybody": ([300], [3], [[0, 1, 2]], 0), "2 folds": ([150, 150], [2, 2], [[0, 2], [0, 1]], 0),
          "3 folds": ([], [], [], 3), "rows 0..128": ([129], [2], [[0, 1]], 11)},
    640: {"everybody": ([640], [5], [[0, 1, 2, 3, 4]], 0), "2 folds": ([320, 320], [3, 3], [[0, 2, 4], [0, 1, 3]], 0),
          "3 folds": ([214, 213, 213], [2, 2, 2], [[0, 3], [0, 2], [0, 2]], 0),
          "129/256/255 dealt": ([129, 256, 255], [2, 2, 2], [[0, 4], [0, 2], [0, 2]], 0),
          "257 late": ([257], [3], [[2, 3, 4]], 23)},
    645: {"5 folds": ([129] * 5, [2] * 5, [[0, 5], [0, 5], [0, 4], [0, 5], [0, 4]], 0)}       # n = 645 has six tile rows
}


@pytest.mark.parametrize("n", [300, 640, 645])
def test_labellings_are_what_the_gpu_tests_say(n):
    labs = kc.labellings(n)
    assert sorted(labs) == sorted(PINNED[n])
    for name, lab in labs.items():
        big_sizes, mts, starts, nsmall = PINNED[n][name]
        sz = kc.sizes(lab)
        assert lab.shape == (n,) and lab.dtype == np.int32 and sz.min() >= 1
        assert [int(m) for m in sz if m > kc.LIMIT] == big_sizes, name
        assert kc.tile_counts(lab) == sorted(mts), name
        assert int(np.sum(sz <= kc.LIMIT)) == nsmall, name
        got = kc.first_tile_rows(lab)
        assert list(got.values()) == starts, name
        for g, rows in got.items():
            assert rows == sorted(rows) and len(rows) == (sz[g] + 127) // 128
    if n == 640:
        rows = lg.tile_rows(labs["129/256/255 dealt"])
        assert rows == [[0, 1, 2, 3, 4]] * 3                 # every group has members in all five tile rows
        late = kc.first_tile_rows(labs["257 late"])
        assert list(late.values()) == [[2, 3, 4]]            # k0 = 2 > 0, and the later blocks start later still
        assert lg.tile_rows(labs["257 late"])[0] == [2, 3, 4]


def test_late_group_and_fold_labels():
    import causalgpslc_jl_amd as gp
    I = kc.late_group()
    assert len(I) == 257 and len(np.unique(I)) == 257 and I[0] // 128 == 2 and I[-1] < 640 and np.all(np.diff(I) > 0)
    for n, K, seed in ((300, 2, 0), (640, 3, 0), (645, 5, 0), (300, 2, 5)):
        assert np.array_equal(kc.fold_labels(n, K, seed), gp.foldLabels(n, K, seed))


@pytest.mark.parametrize("n", [300, 640, 645])
def test_closed_form_against_the_refit_far_inside_the_bound(n):
    """cond(A) <= 41 and cond(C_g) <= 27 on these cases: the device's bound is the floor 1e-10, and the restatement's two sides
    agree within 1e-13 (measured: 4e-15)"""
    c = cases.make_case(n, "UX", False, S=2, seed=kc.SEEDS[n])
    for name, lab in kc.labellings(n).items():
        exp = lg.expected(c, lab)
        for s, e in exp.items():
            errs = lg.errors(e["closed"], e["refit"], e["q"], c["Y"], lab)
            print(n, name, "sample", s, "cond(A) %.3g cond(C) %.3g" % (e["cond"], e["cond_c"]), errs)
            assert e["cond"] <= 41 and e["cond_c"] <= 27.5 and e["tol"] == 1e-10
            assert max(errs) <= 1e-3 * e["tol"], (name, s, errs)


# ---- the front end ------------------------------------------------------------------------------------------------------
CASE = cases.make_case(12, "UX", False, S=2, seed=1)


@pytest.fixture(scope="module")
def gp_front():
    import causalgpslc_jl_amd as gp_
    return gp_


def _kfold_calls(lib):
    return [e for sym, e in lib.calls if sym == "gpslc_y_kfold"]


def test_argument_order_label_compaction_and_keys(gp_front):
    gp = gp_front
    g = cases.gpslc_object(gp, CASE)
    names = ["s2", "s1", "s2", "s10", "s1", "s2", "s2", "s1", "s10", "s10", "s1", "s2"]
    with recording(gp) as lib:
        mean, var, lpd, keys = gp.kfoldPredictive(g, groups=names)
    (e,) = _kfold_calls(lib)
    assert list(keys) == ["s1", "s10", "s2"]
    want = np.array([2, 0, 2, 1, 0, 2, 2, 0, 1, 1, 0, 2], dtype=np.int32)
    assert list(e) == ["ctx", "S", "U", "X_or_null", "Y_or_null", "uyLS", "xyLS", "tyLS", "yScale", "yNoise", "G", "labels",
                       "cvMean", "cvVar", "cvLpd", "logpdf_or_null"]
    assert e["S"] == 2 and e["G"] == 3 and e["labels"] == _array(want)
    assert e["U"] == _array(g.U) and e["X_or_null"] is None and e["Y_or_null"] is None and e["logpdf_or_null"] is None
    assert e["tyLS"] == _array(g.tyLS) and e["yScale"] == _array(g.yScale) and e["yNoise"] == _array(g.yNoise)
    assert mean.shape == (12, 2) and var.shape == (12, 2) and lpd.shape == (3, 2)
    assert e["cvMean"] == _array(mean, with_bytes=False) and e["cvLpd"] == _array(lpd, with_bytes=False)


def test_k_gives_fold_labels_and_overrides_pass_through(gp_front):
    gp = gp_front
    g = cases.gpslc_object(gp, CASE)
    Y2 = np.arange(12.0)
    with recording(gp) as lib:
        *_, keys = gp.kfoldPredictive(g, K=3, seed=4, Y_override=Y2)
        s = gp.kfoldSummary(g, K=3, seed=4)
    a, b = _kfold_calls(lib)
    assert list(keys) == [0, 1, 2] and a["G"] == 3 and a["labels"] == _array(gp.foldLabels(12, 3, 4)) == b["labels"]
    assert a["Y_or_null"] == _array(Y2) and b["Y_or_null"] is None
    assert sorted(s) == ["elpd", "groupwise", "keys", "pit", "zscore"] and s["elpd"].shape == (2,)


def test_refusals_before_any_library_call(gp_front):
    gp = gp_front
    g = cases.gpslc_object(gp, CASE)
    with recording(gp) as lib:
        with pytest.raises(ValueError, match="not both"):
            gp.kfoldPredictive(g, K=2, groups=np.zeros(12, dtype=int))
        with pytest.raises(ValueError, match="kfoldPredictive.*obj"):
            gp.kfoldPredictive(g)                              # no obj column and neither argument
        with pytest.raises(ValueError, match="one label per individual"):
            gp.kfoldPredictive(g, groups=[0, 1])
        with pytest.raises(ValueError):
            gp.kfoldPredictive(g, K=13)
        assert not _kfold_calls(lib)
        g.obj = np.repeat(["b", "a", "c"], 4)
        *_, keys = gp.kfoldPredictive(g)                       # the objects of the data
    (e,) = _kfold_calls(lib)
    assert list(keys) == ["a", "b", "c"] and e["labels"] == _array(np.repeat([1, 0, 2], 4).astype(np.int32))


def test_symbol_is_in_the_binding_table_and_the_library():
    from causalgpslc_jl_amd import _lib
    import causalgpslc_jl_amd as gp
    assert _lib.SIGNATURES["gpslc_y_kfold"] == _lib.SIGNATURES["gpslc_y_lgo"]
    res, args = _lib.SIGNATURES["gpslc_y_kfold"]
    assert res is ctypes.c_int and len(args) == 16 and args[10] is ctypes.c_int32 and args[11] is _lib.c_int32_p
    assert "gpslc_y_kfold" in _lib.header_symbols()
    assert callable(gp.kfoldPredictive) and callable(gp.kfoldSummary) and hasattr(gp.Context, "y_kfold")
    assert "kfoldPredictive" in gp.lgoPredictive.__doc__
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    assert b"\0gpslc_y_kfold\0" in open(_lib.LIB_PATH, "rb").read()
