"""The inputs of tests/test_gpu_node_grad_shapes.py (tests/node_grad_cases.py) checked on the host restatement alone: no GPU.

1. `fits_single_launch`, restated from the documented table, against SmallLayout (csrc/sm_layout.h, compiled and printed by
   tests/c/sm_layout_test.cpp as tests/test_sm_layout.py does) for every n in 1..640 and nF in 0..32, against the arithmetic of
   the gradient's LDS image, and on both sides of the four limits.
2. The sweep's widths cover what they are meant to cover and respect the limits.
3. Every normalised node has sum_f 1 / ls_f^2 = 0.5 and, from n = 32 on, cond(A) >= 10 (the smallest here: 13.8; the nodes at the
   four limits 26 to 81): L, W and A^-1 are dense.  Nodes that share a feature block still share the object.
4. The fp64 restatement against the long-double one: within 1e-3 of the bound on every normalised node (tests/test_node_grad.py's
   criterion; measured: 1.9e-4 at the most), within 1e-2 on the ill-conditioned ones (measured: 2.4e-3), whose cond(A) lies in
   [1e4, 1e8] (1.3e5 to 8.5e5).
5. The inputs see the mistakes the GPU tests are there to catch, each by more than 1e6 bounds: a missing transposed-block
   contribution (dF) and an unmasked padding (dnoise, dscale) on 16 x 16 blocks at 9 to 11 blocks and on 128 x 128 tiles at 3 and 4
   tiles; and, in every call of several nodes, node i evaluated with node 0's target (dscale, dtarget) — a chunk that read the
   wrong set's target."""
import os
import subprocess

import numpy as np
import pytest

import node_grad_cases as nc
import node_grad_restatement as ng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grad_image_fits(tmp_path_factory):
    """{(n, nF): SmallLayout(n, nF, true).bytes() <= kLdsCapBytes} for n in 1..640, nF in 0..32, from the header itself"""
    exe = str(tmp_path_factory.mktemp("sm_layout") / "sm_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "c", "sm_layout_test.cpp")])
    lines = subprocess.check_output([exe], text=True).splitlines()
    head = lines[0].split()
    cap = int(head[head.index("cap") + 1])
    assert cap == nc.LDS_CAP
    out = {}
    for line in lines[1:]:
        w = line.split()
        if w[0] == "small" and w[3] == "1":
            assert w[4] == "bytes"
            out[(int(w[1]), int(w[2]))] = (int(w[5]), int(w[5]) <= cap)
    assert len(out) == 640 * 33
    return out


def test_fits_single_launch_is_the_layouts_limit(grad_image_fits):
    for (n, nF), (size, fits) in grad_image_fits.items():
        assert size == nc.grad_image_bytes(n, nF), (n, nF)
        assert nc.fits_single_launch(n, nF) == fits, (n, nF)


def test_fits_single_launch_on_both_sides_of_the_four_limits():
    assert nc.LIMITS == ((176, 7), (160, 17), (144, 27), (128, 32))
    for n, nF in nc.LIMIT_SINGLE:
        assert nc.fits_single_launch(n, nF) and nc.fits_single_launch(n - 15, nF) and nc.grad_image_bytes(n, nF) <= nc.LDS_CAP
        assert not nc.fits_single_launch(n + 1, nF) and nc.grad_image_bytes(n + 1, nF) > nc.LDS_CAP
        if nF < 32:
            assert not nc.fits_single_launch(n, nF + 1) and nc.grad_image_bytes(n, nF + 1) > nc.LDS_CAP
    assert [nc.fits_single_launch(*s) for s in nc.LIMIT_COLUMN + nc.LIMIT_ROW] == [False] * 7
    assert nc.LIMIT_COLUMN == tuple((n, nF + 1) for n, nF in nc.LIMITS[:3]) and nc.LIMIT_ROW == tuple((n + 1, nF) for n, nF in nc.LIMITS)
    assert not nc.fits_single_launch(128, 33) and not nc.fits_single_launch(177, 0) and nc.fits_single_launch(1, 32)
    assert all(nc.fits_single_launch(176, k[2]) for k in nc.MIXED_176)


def test_the_sweep_covers_the_widths():
    assert sorted(nc.SWEEP_WIDTHS) == list(range(1, 12))
    seen = set()
    for NB, per_size in nc.SWEEP_WIDTHS.items():
        assert nc.sweep_sizes(NB) == (16 * NB - 15, 16 * NB - 7, 16 * NB) and len(per_size) == 3
        assert all(nc.blocks(n) == NB for n in nc.sweep_sizes(NB))
        for n, widths in zip(nc.sweep_sizes(NB), per_size):
            assert len(set(widths)) == 3, (NB, widths)                         # three nodes of different widths
            assert all(nc.fits_single_launch(n, nF) for nF in widths), (NB, n, widths)
            seen.update(widths)
        if NB <= 10:         # the pair sums' short last pass beyond the widths the older tests have
            assert any(nF >= 9 and nF % 4 for widths in per_size for nF in widths), NB
    assert seen >= set(range(9)) | {12, 16}
    assert {17, 27, 32} <= seen                                                # the widest node of 10, 9 and <= 8 blocks
    for NB in nc.SWEEP_WIDTHS:
        for n, keys in nc.sweep_keys(NB):
            assert [(k[1], k[2]) for k in keys] == [(n, nF) for nF in nc.SWEEP_WIDTHS[NB][nc.sweep_sizes(NB).index(n)]]
    keys = nc.all_normalised_keys()
    assert len(set(keys)) == len(keys)


def test_normalised_nodes_are_dense():
    smallest = np.inf
    for key in nc.all_normalised_keys():
        F, ls, scale, noise, target = nc.make(key)
        _, n, nF, seed, fseed = (tuple(key) + (None,))[:5]
        raw = ng.random_node(n, nF, seed, fseed)
        assert nc.make(key) is nc.make(list(key)) and F is raw[0] and target is raw[4] and (scale, noise) == raw[2:4]
        if nF == 0:
            assert F is None and ls is None
            continue
        assert F.shape == (n, nF) and abs(np.sum(1.0 / ls ** 2) - 0.5) <= 1e-14
        assert np.allclose(ls / raw[1], ls[0] / raw[1][0], rtol=1e-15, atol=0)      # ONE factor
        if n >= 32:
            cond = nc.expected(key)[3]
            smallest = min(smallest, cond)
            assert cond >= 10, (key, cond)
    print("smallest cond(A) of a normalised node with n >= 32: %.3g" % smallest)
    for shared in (nc.CHUNK_SHARED, nc.TILE_SHARED):
        nodes = [nc.make(k) for k in shared]
        assert nodes[0][0] is nodes[1][0] is nodes[2][0]
        assert len({tuple(nd[1]) for nd in nodes}) == 3 and len({nd[4].tobytes() for nd in nodes}) == 3
    plain = ng.random_node(40, 0, 1)
    assert nc.normalised(plain) is plain


GROUPS = {"sweep %d" % NB: [k for _, ks in nc.sweep_keys(NB) for k in ks] for NB in nc.SWEEP_WIDTHS}
GROUPS["limits"] = [nc.limit_key(*s) for s in nc.LIMIT_SINGLE + nc.LIMIT_COLUMN + nc.LIMIT_ROW] + nc.MIXED_176
GROUPS["tiles"] = [k for n in nc.TILE_SIZES for k in nc.tile_keys(n)] + nc.TILE_SHARED
GROUPS["calls of several nodes"] = nc.CHUNK_KEYS + nc.CHUNK_SHARED + nc.MANY_129 + nc.MANY_5


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_fp64_restatement_against_long_double(group):
    worst = 0.0
    for key in GROUPS[group]:
        gl, sl, tol, cond = nc.expected(key)
        g64, _ = ng.gradient(nc.make(key), np.float64)
        err = nc.fractions(g64, gl, sl)
        worst = max(worst, max(err.values()) / tol)
        assert max(err.values()) <= 1e-3 * tol, (key, err, tol)
        if key[2]:
            assert np.all(np.abs(gl["dF"].sum(0)) <= tol * sl["dF"].sum(0)), (key, "shift identity")
    print(group, "fp64 error / bound, worst: %.3g" % worst)


@pytest.mark.parametrize("n,noise", nc.ILL)
def test_ill_conditioned_nodes(n, noise):
    F, ls, scale, nz, target = nc.ill_node(n, noise)
    assert nc.ill_node(n, noise) is nc.make(("ill", n, noise))
    assert F.shape == (n, 3) and np.array_equal(ls, [6.0, 6.0, 6.0]) and scale == 1.0 and nz == noise and target.shape == (n,)
    gl, sl, tol, cond = nc.expected(("ill", n, noise))
    assert 1e4 <= cond <= 1e8 and tol == 1e-14 * cond > 1e-10
    g64, _ = ng.gradient(nc.ill_node(n, noise), np.float64)
    err = nc.fractions(g64, gl, sl)
    print("n", n, "noise", noise, "cond %.3g" % cond, "fp64 error / bound:", {k: v / tol for k, v in err.items()})
    assert max(err.values()) <= 1e-2 * tol, err


def _moved(key, **mutation):
    node = nc.make(key)
    tol = ng.node_tolerance(node)[0]
    good, sc = ng.gradient(node)
    move = nc.fractions(ng.gradient(node, **mutation)[0], good, sc)
    print(key, mutation, "moves, in bounds:", {k: v / tol for k, v in move.items()})
    return move, tol


@pytest.mark.parametrize("key,block", [(nc.limit_key(144, 27), 16), (nc.limit_key(176, 7), 16),
                                       (nc.tile_keys(257)[0], 128), (nc.tile_keys(385)[0], 128)])
def test_the_inputs_can_see_a_missing_transposed_block(key, block):
    move, tol = _moved(key, block=block, no_transpose=True)
    assert move["dF"] > 1e6 * tol


@pytest.mark.parametrize("key,block", [(nc.limit_key(129, 32), 16), (nc.limit_key(161, 17), 16), (nc.tile_keys(257)[0], 128)])
def test_the_inputs_can_see_an_unmasked_padding(key, block):
    move, tol = _moved(key, block=block, no_mask=True)
    assert move["dnoise"] > 1e6 * tol and move["dscale"] > 1e6 * tol


@pytest.mark.parametrize("call", sorted(nc.MULTI_NODE_CALLS))
def test_the_inputs_can_see_the_wrong_sets_target(call):
    keys = nc.MULTI_NODE_CALLS[call]
    first = nc.make(keys[0])[4]
    for key in keys[1:]:
        gl, sl, tol, _ = nc.expected(key)
        wrong, _ = ng.gradient(nc.with_target(nc.make(key), first))
        move = nc.fractions(wrong, gl, sl)
        print(call, key, "with node 0's target, in bounds:", {k: v / tol for k, v in move.items()})
        assert move["dscale"] > 1e6 * tol and move["dtarget"] > 1e6 * tol, (key, move)
