"""Inputs of tests/test_gpu_node_grad_shapes.py and the CPU checks of those inputs (tests/test_node_grad_cases.py): no GPU.

A node is named by a KEY, a tuple `make` turns into (F, ls, scale, noise, target) and `expected` into its long-double gradient —
one object and one reference per key and session, as node_grad_restatement.random_node keeps them:

    ("n", n, nF, seed[, fseed])   random_node(n, nF, seed, fseed) through `normalised`
    ("ill", n, noise)             `ill_node(n, noise)`

`normalised` rescales a node's lengthscales so that sum_f 1 / ls_f^2 = 0.5: two standard-normal individuals then sit at an expected
squared scaled distance of 1 whatever the width, K_rc / scale is of order e^-1, and L, W = L^-1 and A^-1 are dense.  With
random_node's own lengthscales on (1.5, 3) a node of 27 or 32 columns has cond(A) = 1.09 or 1.01: A is the identity to many digits
and the block-column back-substitution and the W^T W chains only show in terms of order K^2.

The tables below are the shapes of the GPU tests, kept here so that the CPU checks see the same nodes."""
import functools

import numpy as np

import node_grad_restatement as ng

LD = np.longdouble
OUT = ng.OUTPUTS
BLOCK = 16
LDS_CAP = 160 * 1024


# ---- the single launch's limits, restated from the documented table --------------------------------------------------------------

def blocks(n):
    return -(-n // BLOCK)


def fits_single_launch(n, nF):
    """the documented limits of the gradient's single launch: NB = ceil(n / 16) blocks hold up to 7 (NB = 11), 17 (10), 27 (9) or
    32 (NB <= 8) feature columns; nothing beyond 11 blocks or 32 columns"""
    NB = blocks(n)
    if n < 1 or nF < 0 or nF > 32 or NB > 11:
        return False
    return nF <= {11: 7, 10: 17, 9: 27}.get(NB, 32)


def grad_image_bytes(n, nF):
    """the arithmetic of the gradient's LDS image: lower blocks, four vectors, the broadcast lines, and per feature column the
    scaled and the raw copy, a partial per block row and the lengthscale"""
    NB = blocks(n)
    NP = BLOCK * NB
    return (NB * (NB + 1) // 2 * 256 + 4 * NP + 128 + nF * (2 * NP + NB + 1)) * 8


LIMITS = ((176, 7), (160, 17), (144, 27), (128, 32))


# ---- nodes -----------------------------------------------------------------------------------------------------------------------

def normalised(node):
    """the node with its lengthscales times ONE factor so that sum_f 1 / ls_f^2 = 0.5; a node without features as it is.  The
    feature block stays the same object: nodes that share one still share one pointer."""
    F, ls, scale, noise, target = node
    if ls is None or np.size(ls) == 0:
        return node
    ls = np.asarray(ls, dtype=np.float64)
    return (F, ls * np.sqrt(2.0 * np.sum(1.0 / ls ** 2)), scale, noise, target)


def ill_node(n, noise):
    """three standard-normal columns, every lengthscale 6, scale 1 and a small noise: cond(A) of 1e5 to 1e6 at n = 150 and 200"""
    return make(("ill", n, float(noise)))


def make(key):
    """the node of `key` — one object per key and session, however the key is spelled"""
    return _make(_canon(key))


def expected(key):
    """(grads, scales, tol, cond) of the node in long double — computed once per session"""
    return _expected(_canon(key))


def _canon(key):
    key = tuple(key)
    if key[0] == "n":
        return key + (None,) * (5 - len(key))
    assert key[0] == "ill" and len(key) == 3, key
    return ("ill", int(key[1]), float(key[2]))


@functools.lru_cache(maxsize=None)
def _make(key):
    if key[0] == "n":
        return normalised(ng.random_node(*key[1:]))
    _, n, noise = key
    rng = np.random.default_rng((7, n))
    return (np.asfortranarray(rng.standard_normal((n, 3))), np.full(3, 6.0), 1.0, noise, rng.standard_normal(n))


@functools.lru_cache(maxsize=None)
def _expected(key):
    node = _make(key)
    g, s = ng.gradient(node, LD)
    tol, cond = ng.node_tolerance(node)
    return g, s, tol, cond


def with_target(node, target):
    return node[:4] + (target,)


def fractions(got, ref, scales):
    """{output: max over its elements of |got - ref| / scale}, compared in long double — node_grad_restatement.errors with the
    elements of scale 0 (a node of one individual has no pairs: dF, dls and their scales are exact zeros) spelled out: 0 where the
    output is the reference, inf where it is not.  An output is inside its bound when its fraction is <= tol."""
    out = {}
    for k in OUT:
        if got.get(k) is None:
            continue
        g, r, s = (np.asarray(x, dtype=LD) for x in (got[k], ref[k], scales[k]))
        assert g.shape == r.shape, (k, g.shape, r.shape)
        d = np.abs(g - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            fr = np.where(s > 0, d / s, np.where(d == 0, 0.0, np.inf))
        out[k] = float(np.max(fr)) if g.size else 0.0
    return out


# ---- the shapes of the GPU tests -------------------------------------------------------------------------------------------------

# block-count sweep: per NB the widths of the three nodes of the calls at n = 16 NB - 15, 16 NB - 7 and 16 NB
SWEEP_WIDTHS = {
    1: ((0, 1, 9), (2, 5, 16), (3, 32, 6)),
    2: ((4, 7, 13), (8, 12, 0), (1, 11, 31)),
    3: ((2, 6, 10), (0, 16, 21), (5, 8, 30)),
    4: ((3, 7, 14), (1, 12, 29), (0, 4, 18)),
    5: ((6, 8, 15), (2, 16, 26), (0, 5, 32)),
    6: ((1, 7, 17), (3, 12, 23), (4, 9, 32)),
    7: ((0, 8, 19), (2, 6, 16), (5, 11, 28)),
    8: ((3, 10, 32), (1, 12, 22), (7, 4, 31)),
    9: ((27, 4, 10), (1, 16, 22), (8, 12, 25)),
    10: ((0, 9, 17), (5, 12, 16), (2, 13, 17)),
    11: ((0, 3, 7), (1, 4, 6), (2, 5, 7)),
}


def sweep_sizes(NB):
    return (BLOCK * NB - 15, BLOCK * NB - 7, BLOCK * NB)


def sweep_keys(NB):
    """[(n, [key, key, key])] of block count NB"""
    return [(n, [("n", n, nF, 1500 * NB + 10 * j + i) for i, nF in enumerate(widths)])
            for j, (n, widths) in enumerate(zip(sweep_sizes(NB), SWEEP_WIDTHS[NB]))]


def limit_key(n, nF):
    return ("n", n, nF, 2000 + n + nF)


LIMIT_SINGLE = LIMITS
LIMIT_COLUMN = ((176, 8), (160, 18), (144, 28))                 # one column more: tiled
LIMIT_ROW = ((177, 7), (161, 17), (145, 27), (129, 32))         # one row more: tiled
MIXED_176 = [("n", 176, nF, 2500 + i) for i, nF in enumerate((7, 0, 3))]

ILL = ((150, 1e-3), (150, 2e-4), (200, 1e-3), (200, 2e-4))      # n = 150: the single launch; n = 200: tiled

TILE_SIZES = (256, 257, 300, 385)                                # 2, 3, 3 and 4 tiles of 128 per side


def tile_keys(n):
    return [("n", n, nF, 3000 + n + i) for i, nF in enumerate((3, 0, 8) + ((32,) if n == 257 else ()))]


def shared_keys(n, seed, nF=2):
    """three nodes on ONE feature block, the last one its owner"""
    return [("n", n, nF, seed + 1, seed), ("n", n, nF, seed + 2, seed), ("n", n, nF, seed)]


# The featureless node's seed is picked: without features dscale sees the target only through (1' target)^2, one part in n of its
# scale, so a standard-normal target of another node moves it by 1e4 to 1e5 bounds.  Seed 7729's target sums to -60 (4.2 sigma):
# read with node 0's target its dscale moves by 1.8e6 bounds, which is what the CPU check asks of every node of these calls.
CHUNK_KEYS = [("n", 200, nF, seed) for nF, seed in ((3, 4000), (8, 4001), (0, 7729), (16, 4003), (1, 4004))]
CHUNK_SHARED = shared_keys(200, 4100)
TILE_SHARED = shared_keys(300, 3900)

MANY_129 = [("n", 129, nF, 5000 + i) for i, nF in enumerate((0, 1, 3, 8, 16))]          # 260 nodes cycle over these
MANY_5 = [("n", 5, nF, 5100 + i) for i, nF in enumerate((0, 1, 2, 3, 0, 1, 2, 3))]      # 4097 nodes cycle over these
MULTI_NODE_CALLS = {"chunks": CHUNK_KEYS, "chunks, shared block": CHUNK_SHARED, "260 nodes": MANY_129, "4097 nodes": MANY_5}


def all_normalised_keys():
    keys = [k for NB in SWEEP_WIDTHS for _, ks in sweep_keys(NB) for k in ks]
    keys += [limit_key(n, nF) for n, nF in LIMIT_SINGLE + LIMIT_COLUMN + LIMIT_ROW] + MIXED_176
    keys += [k for n in TILE_SIZES for k in tile_keys(n)] + TILE_SHARED
    keys += CHUNK_KEYS + CHUNK_SHARED + MANY_129 + MANY_5
    return keys
