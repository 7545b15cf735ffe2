"""The labellings of the K-fold tests (tests/test_kfold.py pins them on the CPU, tests/test_gpu_kfold.py runs them; test
infrastructure).  gpslc_y_kfold sends a group of m <= 128 members through lgo_group_kernel and a larger one through the tiled
path: C as an mt x mt triangle of tiles, mt = ceil(m / 128), the chain of tile (p, q) starting at the tile row of the first
member of row block p.  The shapes are the smallest that reach each layout: n = 300 (three tiles, the last ragged), n = 640
(five tiles, no padding), n = 645 (five folds of 129)."""
import numpy as np

import lgo_restatement as lg

SEEDS = {300: 701, 640: 700, 645: 702}                      # cases.make_case(n, "UX", False, S=2, seed=SEEDS[n])
LIMIT = 128                                                 # LGO_MAX_GROUP


def fold_labels(n, K, seed=0):
    """causalgpslc_jl_amd.foldLabels, restated (tests/test_kfold.py asserts they agree)"""
    labels = np.empty(n, dtype=np.int32)
    labels[np.random.default_rng(seed).permutation(n)] = np.arange(n, dtype=np.int32) % K
    return labels


def dealt(n, sizes, seed):
    """groups of `sizes` dealt through a fixed permutation of the rows: every large group has members in every tile row"""
    assert sum(sizes) == n
    lab = np.empty(n, dtype=np.int64)
    lab[np.random.default_rng(seed).permutation(n)] = np.repeat(np.arange(len(sizes)), sizes)
    return lab.astype(np.int32)


def late_group(n=640, lo=256, m=257, seed=643):
    """rows of one group of m members scattered over the rows lo .. n - 1: its first member lies in tile row lo / 128 > 0
    (tests/test_kfold.py pins it), ascending"""
    return np.sort(lo + np.random.default_rng(seed).permutation(n - lo)[:m])


def labellings(n):
    """name -> labels (n,) of the refit comparison"""
    if n == 300:
        return {"everybody": lg.one_group(n), "2 folds": fold_labels(n, 2), "3 folds": fold_labels(n, 3),
                "rows 0..128": lg.with_block(n, 0, 129)}
    if n == 640:
        return {"everybody": lg.one_group(n), "2 folds": fold_labels(n, 2), "3 folds": fold_labels(n, 3),
                "129/256/255 dealt": dealt(n, (129, 256, 255), 644), "257 late": lg.beside(n, late_group(), 17)}
    if n == 645:
        return {"5 folds": fold_labels(n, 5)}
    raise KeyError(n)


def sizes(labels):
    return np.bincount(labels)


def tile_counts(labels):
    """mt of every group beyond LIMIT members"""
    return sorted(int((m + 127) // 128) for m in sizes(labels) if m > LIMIT)


def first_tile_rows(labels):
    """per group beyond LIMIT members: the tile row every row block's chain starts at (block p: that of member 128 p)"""
    return {g: [int(I[128 * p] // 128) for p in range((len(I) + 127) // 128)]
            for g, I in enumerate(lg.members_of(labels)) if len(I) > LIMIT}
