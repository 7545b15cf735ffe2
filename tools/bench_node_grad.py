#!/usr/bin/env python3
"""Cost of the fused whole-model gradient (gpslc_nodes_logpdf_grad) on one MI355X, in one run:

  * the node set of a U move — nX = 4 `:X => k => :X` nodes on F = U, `:T` on [U | X], `:Y` on [U | X | T]; nU = 1 and 2 — at
    n = 150 and at the largest n the single launch takes for that set: microseconds per call of gpslc_nodes_logpdf_grad and of
    gpslc_nodes_logpdf;
  * the `:Y` node alone through gpslc_nodes_logpdf_grad (single launch) against gpslc_y_logpdf_grad with S = 1, which takes the
    tiled path at every n.

Method: the C entry points with the arguments marshalled once (what a Julia ccall sees); every call ends in the library's own
stream synchronisation, so a host clock around `reps` calls measures device-complete calls.  Every variant is warmed up, then
the variants of a row are timed in alternation over `rounds` rounds; the table gives the median round and the spread.
Prints a markdown table; `--out FILE` also writes it there."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import causalgpslc_jl_amd as gp   # noqa: E402
from causalgpslc_jl_amd import api   # noqa: E402

NX = 4


def largest_single_launch_n(nF):
    """the header's table: the gradient's LDS image (packed 16 x 16 blocks, four vectors, scaled and raw features, one
    lengthscale partial per block row, the lengthscales, the pivot chains' broadcast lines) within 160 KiB"""
    best = 0
    for n in range(1, 400):
        NB = (n + 15) // 16
        NP = 16 * NB
        if (NB * (NB + 1) // 2 * 256 + 4 * NP + 128 + 2 * nF * NP + nF * NB + nF) * 8 <= 160 * 1024:
            best = n
    return best


def move_nodes(n, nU, rng):
    U = np.asfortranarray(rng.standard_normal((n, nU)))
    X = np.asfortranarray(rng.standard_normal((n, NX)))
    T, Y = rng.standard_normal(n), rng.standard_normal(n)
    ls = lambda k: rng.uniform(1.5, 3.0, k)     # noqa: E731
    nodes = [(U, ls(nU), 1.1, 0.5, np.ascontiguousarray(X[:, k])) for k in range(NX)]
    nodes.append((np.asfortranarray(np.column_stack([U, X])), ls(nU + NX), 0.9, 0.6, T))
    y = (np.asfortranarray(np.column_stack([U, X, T])), ls(nU + NX + 1), 1.3, 0.4, Y)
    return nodes + [y], (U, X, T, Y, y)


def timed(fns, reps, rounds):
    """{name: sorted microseconds per call, one figure per round}, the variants alternating inside every round"""
    for fn in fns.values():
        for _ in range(20):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            out[k].append((time.perf_counter() - t0) / reps * 1e6)
    return {k: sorted(v) for k, v in out.items()}


def fmt(v):
    return f"{v[len(v) // 2]:.1f} ({v[0]:.1f} – {v[-1]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = lambda x: x.ctypes.data_as(C.c_void_p)     # noqa: E731
    lines = ["| case | n | widest node | `gpslc_nodes_logpdf_grad`, µs | `gpslc_nodes_logpdf`, µs | ratio |", "|---|---|---|---|---|---|"]
    ylines = ["| n | `:Y` through `gpslc_nodes_logpdf_grad`, µs | `gpslc_y_logpdf_grad`, S = 1, µs | tiled / single launch |", "|---|---|---|---|"]
    for nU in (1, 2):
        for n in (150, largest_single_launch_n(nU + NX + 1)):
            rng = np.random.default_rng(1000 * nU + n)
            nodes, (U, X, T, Y, ynode) = move_nodes(n, nU, rng)
            cnt = len(nodes)
            ctx = gp.Context(n, NX, nU, profile=True)
            ctx.set_data(X, T, Y)
            arr, _keep = api._marshal_nodes(nodes, ctx)
            tot = sum(nd[0].shape[1] for nd in nodes)
            dF, dls, dsc, dno, dtg, lp = (np.empty(k) for k in (n * tot, tot, cnt, cnt, n * cnt, cnt))
            lib, h, parr = ctx.lib, ctx.h, C.cast(arr, C.c_void_p)
            grad = lambda: lib.gpslc_nodes_logpdf_grad(h, cnt, parr, p(dF), p(dls), p(dsc), p(dno), p(dtg), p(lp))     # noqa: E731
            score = lambda: lib.gpslc_nodes_logpdf(h, cnt, parr, p(lp))     # noqa: E731
            ctx.profile_reset()
            assert grad() == 0 and score() == 0
            assert sum(ctx.profile_get(k)[0] for k in (0, 1, 4)) == 0, "the single launch was expected"
            t = timed({"grad": grad, "score": score}, a.reps, a.rounds)
            lines.append(f"| U move, nU = {nU}: {NX} X nodes, T, Y | {n} | nF = {nU + NX + 1} | {fmt(t['grad'])} | {fmt(t['score'])} | "
                         f"{t['grad'][len(t['grad']) // 2] / t['score'][len(t['score']) // 2]:.2f} |")
            # the :Y node alone, against the outcome call on the tiled path
            yarr, _keep_y = api._marshal_nodes([ynode], ctx)
            pyarr = C.cast(yarr, C.c_void_p)
            F = nU + NX + 1
            ydF, ydls, ys1, yn1, ydt = (np.empty(k) for k in (n * F, F, 1, 1, n))
            single = lambda: lib.gpslc_nodes_logpdf_grad(h, 1, pyarr, p(ydF), p(ydls), p(ys1), p(yn1), p(ydt), p(lp))     # noqa: E731
            lsy = ynode[1]
            uy, xy, ty = np.ascontiguousarray(lsy[:nU]), np.ascontiguousarray(lsy[nU:nU + NX]), np.ascontiguousarray(lsy[-1:])
            sc, no = np.array([ynode[2]]), np.array([ynode[3]])
            gU, guy, gxy, gty, gsc, gno, gY = (np.empty(k) for k in (n * nU, nU, NX, 1, 1, 1, n))
            tiled = lambda: lib.gpslc_y_logpdf_grad(h, 1, p(U), None, None, p(uy), p(xy), p(ty), p(sc), p(no), p(gU), p(guy), p(gxy),     # noqa: E731
                                                    p(gty), p(gsc), p(gno), p(gY), p(lp))
            assert single() == 0 and tiled() == 0
            assert np.allclose(ydF[:n * nU], gU, rtol=1e-6, atol=1e-9) and np.allclose(ydt, gY, rtol=1e-6, atol=1e-9)
            t = timed({"single": single, "tiled": tiled}, max(a.reps // 3, 20), a.rounds)
            ylines.append(f"| {n} (nU = {nU}) | {fmt(t['single'])} | {fmt(t['tiled'])} | "
                          f"{t['tiled'][len(t['tiled']) // 2] / t['single'][len(t['single']) // 2]:.1f} |")
    text = "\n".join([f"median of {a.rounds} rounds of {a.reps} device-synchronised calls (min – max), after 20 warm-up calls per variant; "
                      "the variants of a row alternate inside every round; the `:Y` rows time a third of the calls per round", ""] + lines + [""] + ylines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
