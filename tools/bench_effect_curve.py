"""The joint covariance of an effect curve (effectCurve, gpslc_predict_curve) against the weighted call with the same levels and
weight columns, through the Python mirror's call path (causalgpslc_jl_amd.api._predict_curve with and without covW).

For N in {1024, 4096} (S = 1024 posterior samples), L in {4, 32, 101} levels and G in {1, 4} weight columns: every shape is run
once to warm up (workspace, kernel loading), then timed `--reps` times (best of); a call returns only after its results are on
the host, so every timing is device-synchronised and the curve call's includes the S x L x L x G covariance's copy.  The
weighted call is measured twice, before and after the curve call, so that the table shows the spread of two plain measurements
next to the difference it is compared with.  A curve call adds, per sample, the prior terms (one workgroup per weight column)
and one Gram pass over the solved right-hand-side rows (one workgroup per 16 x 16 block of level pairs of the same column).
Last, what the diagonal blocks of the same covariance cost without the feature: ITEDistributions (the full n x n CovITE per
sample and level) at the same N, S = `--S-cov`, per sample and level.  Prints one JSON line per shape and a summary table.

    python tools/bench_effect_curve.py [--sizes 1024,4096] [--levels 4,32,101] [--groups 1,4] [--S 1024] [--reps 2] [--S-cov 8]
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
    ap.add_argument("--levels", default="4,32,101")
    ap.add_argument("--groups", default="1,4")
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
            xs = np.linspace(-1.0, 1.0, L)
            for G in (int(v) for v in args.groups.split(",")):
                W = np.vstack([rng.random(n) < 0.4 for _ in range(G)])       # G group masks
                t_w1 = timed(lambda: gp.api._predict_curve(g, xs, weights=W, want_cov=False), args.reps)
                t_c = timed(lambda: gp.api._predict_curve(g, xs, weights=W), args.reps)
                t_w2 = timed(lambda: gp.api._predict_curve(g, xs, weights=W, want_cov=False), args.reps)
                t_w = min(t_w1, t_w2)
                row = dict(n=n, S=args.S, L=L, G=G, weighted_s=[t_w1, t_w2], curve_s=t_c,
                           weighted_samples_per_s=[args.S / t_w1, args.S / t_w2], curve_samples_per_s=args.S / t_c,
                           extra_us_per_sample=1e6 * (t_c - t_w) / args.S,
                           weighted_spread_us_per_sample=1e6 * abs(t_w1 - t_w2) / args.S)
                rows.append(row)
                print(json.dumps(row), flush=True)
        g.ctx().close()
        # the diagonal blocks alone today: the full CovITE of ITEDistributions, one call per level
        gc = make_object(gp, n, args.S_cov)
        t_cov = timed(lambda: gp.ITEDistributions(gc, 0.5), 1)
        cov = dict(n=n, S=args.S_cov, ite_distributions_s=t_cov, us_per_sample_and_level=1e6 * t_cov / args.S_cov)
        cov_rows.append(cov)
        print(json.dumps(cov), flush=True)
        gc.ctx().close()
    print("\n| N | L | G | weighted call, samples/s (two measurements) | curve call, samples/s | extra per sample (us) | "
          "spread of the weighted measurements (us per sample) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["weighted_samples_per_s"]
        print(f"| {r['n']} | {r['L']} | {r['G']} | {a:,.0f} / {b:,.0f} | {r['curve_samples_per_s']:,.0f} | "
              f"{r['extra_us_per_sample']:+.1f} | {r['weighted_spread_us_per_sample']:.1f} |")
    print("\n| N | ITEDistributions (full CovITE, one level), S | seconds | us per sample and level |")
    print("|---|---|---|---|")
    for r in cov_rows:
        print(f"| {r['n']} | {r['S']} | {r['ite_distributions_s']:.3f} | {r['us_per_sample_and_level']:,.0f} |")


if __name__ == "__main__":
    main()
