"""Weighted average effects (predict(..., weights=)) against the plain call through the public API (causalgpslc_jl_amd.predict).

For N in {1024, 4096} (S = 1024 posterior samples), L in {1, 4} levels and G in {1, 4, 16} weight columns, ordinary estimand
and contrast: every shape is run once to warm up (workspace, kernel loading), then timed `--reps` times (best of); predict()
returns only after the results are on the host, so every timing is device-synchronised.  All calls ask for MeanITE.  The plain
call with the same L is measured twice, before and after the weighted calls, so that the table shows the spread of repeated
plain calls next to the difference it is compared with.  A weighted call adds one pass over the pairs per sample (the
weighted-sum kernel, all G columns and L levels together) and L G - L right-hand-side rows.  Last, what the same variance costs
without the feature: ITEDistributions (the full n x n CovITE per sample) at the same N, S = `--S-cov`, per sample.
Prints one JSON line per shape and a summary table.

    python tools/bench_group_weights.py [--sizes 1024,4096] [--levels 1,4] [--groups 1,4,16] [--S 1024] [--reps 2] [--S-cov 8]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--levels", default="1,4")
    ap.add_argument("--groups", default="1,4,16")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--S-cov", type=int, default=8)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    rows, cov_rows = [], []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        rng = np.random.default_rng(n)
        for L in (int(v) for v in args.levels.split(",")):
            xs = np.linspace(-0.5, 0.5, L)
            base = xs - 0.75                   # every pair 0.75 apart
            t_p1 = timed(lambda: gp.predict(g, xs, want_mean_ite=True), args.reps)
            mid = []
            for G in (int(v) for v in args.groups.split(",")):
                W = np.vstack([rng.random(n) < 0.4 for _ in range(G)])       # G group masks
                t_o = timed(lambda: gp.predict(g, xs, want_mean_ite=True, weights=W), args.reps)
                t_c = timed(lambda: gp.predict(g, xs, want_mean_ite=True, baseline=base, weights=W), args.reps)
                mid.append((G, t_o, t_c))
            t_p2 = timed(lambda: gp.predict(g, xs, want_mean_ite=True), args.reps)
            t_p = min(t_p1, t_p2)
            for G, t_o, t_c in mid:
                row = dict(n=n, S=args.S, L=L, G=G, plain_s=[t_p1, t_p2], weighted_s=t_o, weighted_contrast_s=t_c,
                           plain_samples_per_s=[args.S / t_p1, args.S / t_p2], weighted_samples_per_s=args.S / t_o,
                           weighted_contrast_samples_per_s=args.S / t_c,
                           extra_us_per_sample=1e6 * (t_o - t_p) / args.S, extra_contrast_us_per_sample=1e6 * (t_c - t_p) / args.S,
                           plain_spread_us_per_sample=1e6 * abs(t_p1 - t_p2) / args.S)
                rows.append(row)
                print(json.dumps(row), flush=True)
        g.ctx().close()
        # the same variance today: the full CovITE of ITEDistributions (S x n x n on the host: 134 MB per sample at N = 4096)
        gc = make_object(gp, n, args.S_cov)
        t_cov = timed(lambda: gp.ITEDistributions(gc, 0.5), 1)
        cov = dict(n=n, S=args.S_cov, ite_distributions_s=t_cov, us_per_sample=1e6 * t_cov / args.S_cov)
        cov_rows.append(cov)
        print(json.dumps(cov), flush=True)
        gc.ctx().close()
    print("\n| N | L | G | plain call, samples/s (two measurements) | weighted, samples/s | weighted contrast, samples/s | extra per "
          "sample (us) | extra per sample, contrast (us) | spread of the plain measurements (us per sample) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["plain_samples_per_s"]
        print(f"| {r['n']} | {r['L']} | {r['G']} | {a:,.0f} / {b:,.0f} | {r['weighted_samples_per_s']:,.0f} | "
              f"{r['weighted_contrast_samples_per_s']:,.0f} | {r['extra_us_per_sample']:+.1f} | "
              f"{r['extra_contrast_us_per_sample']:+.1f} | {r['plain_spread_us_per_sample']:.1f} |")
    print("\n| N | ITEDistributions (full CovITE), S | seconds | us per sample |")
    print("|---|---|---|---|")
    for r in cov_rows:
        print(f"| {r['n']} | {r['S']} | {r['ite_distributions_s']:.3f} | {r['us_per_sample']:,.0f} |")


if __name__ == "__main__":
    main()
