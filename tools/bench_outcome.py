"""Outcome levels (predict(..., outcome=True)) against ordinary levels through the public API (causalgpslc_jl_amd.predict), scalar
and per-individual.

For N in {1024, 4096} (S = 1024 posterior samples) and L in {1, 4, 16} levels: every shape is run once to warm up (workspace,
kernel loading), then timed `--reps` times (best of); predict() returns only after the results are on the host, so every
timing is device-synchronised.  Scalar levels: the ordinary call is measured twice, before and after the outcome call, so that
the table shows the spread of repeated ordinary calls next to the difference it is compared with — an outcome level runs the
same launches as an ordinary level and differs by O(N L) work per sample only.  Vector levels: the ordinary vector call of
tools/bench_vector_intervention.py (same levels) next to the outcome vector call, again ordinary / outcome / ordinary; the
outcome form evaluates the same exps per pair and fewer terms.  Prints one JSON line per shape and two summary tables.

    python tools/bench_outcome.py [--sizes 1024,4096] [--levels 1,4,16] [--S 1024] [--reps 2] [--no-vector]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_vector_intervention import make_object, timed   # noqa: E402


def sandwich(gp, g, levels, reps, S, L):
    """ordinary, outcome, ordinary for one set of levels: the row of the table."""
    t1 = timed(lambda: gp.predict(g, levels, want_mean_ite=True), reps)
    to = timed(lambda: gp.predict(g, levels, want_mean_ite=True, outcome=True), reps)
    t2 = timed(lambda: gp.predict(g, levels, want_mean_ite=True), reps)
    t = min(t1, t2)
    return dict(ordinary_s=[t1, t2], outcome_s=to, ordinary_samples_per_s=[S / t1, S / t2], outcome_samples_per_s=S / to,
                extra_us_per_sample_level=1e6 * (to - t) / (S * L),
                ordinary_spread_us_per_sample_level=1e6 * abs(t1 - t2) / (S * L))


def table(rows, kind):
    print(f"\n| N | L | ordinary {kind} levels, samples/s (two measurements) | outcome {kind} levels, samples/s | extra per outcome "
          "level and sample (us) | spread of the ordinary measurements, same unit (us) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["ordinary_samples_per_s"]
        print(f"| {r['n']} | {r['L']} | {a:,.0f} / {b:,.0f} | {r['outcome_samples_per_s']:,.0f} | "
              f"{r['extra_us_per_sample_level']:+.2f} | {r['ordinary_spread_us_per_sample_level']:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--levels", default="1,4,16")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-vector", action="store_true")
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    scalar, vector = [], []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        rng = np.random.default_rng(n)
        for L in (int(v) for v in args.levels.split(",")):
            xs = np.linspace(-0.5, 0.5, L)
            row = dict(n=n, S=args.S, L=L, kind="scalar", **sandwich(gp, g, xs, args.reps, args.S, L))
            scalar.append(row)
            print(json.dumps(row), flush=True)
            if args.no_vector:
                continue
            # the vector levels of tools/bench_vector_intervention.py: everyone shifted, or half the individuals left as observed
            D = np.stack([np.where(rng.random(n) < 0.5, g.T, g.T + x) if l % 2 else g.T + x for l, x in enumerate(xs)])
            row = dict(n=n, S=args.S, L=L, kind="vector", **sandwich(gp, g, D, args.reps, args.S, L))
            vector.append(row)
            print(json.dumps(row), flush=True)
        g.ctx().close()
    table(scalar, "scalar")
    if vector:
        table(vector, "vector")


if __name__ == "__main__":
    main()
