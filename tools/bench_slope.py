"""Slope levels (predict(..., slope=True)) against ordinary scalar levels through the public API (causalgpslc_jl_amd.predict).

For N in {1024, 4096} (S = 1024 posterior samples) and L in {1, 4, 16} levels: every shape is run once to warm up (workspace,
kernel loading), then timed `--reps` times (best of); predict() returns only after the results are on the host, so every
timing is device-synchronised.  The scalar call is measured twice, before and after the slope call, so that the table shows
the spread of repeated scalar calls next to the difference it is compared with: a slope level runs the same launches as a
scalar level and differs by O(N L) work per sample only.  Prints one JSON line per shape and a summary table.

    python tools/bench_slope.py [--sizes 1024,4096] [--levels 1,4,16] [--S 1024] [--reps 2]
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
    ap.add_argument("--levels", default="1,4,16")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        for L in (int(v) for v in args.levels.split(",")):
            xs = np.linspace(-0.5, 0.5, L)
            t_s1 = timed(lambda: gp.predict(g, xs, want_mean_ite=True), args.reps)
            t_d = timed(lambda: gp.predict(g, xs, want_mean_ite=True, slope=True), args.reps)
            t_s2 = timed(lambda: gp.predict(g, xs, want_mean_ite=True), args.reps)
            t_s = min(t_s1, t_s2)
            row = dict(n=n, S=args.S, L=L, scalar_s=[t_s1, t_s2], slope_s=t_d,
                       scalar_samples_per_s=[args.S / t_s1, args.S / t_s2], slope_samples_per_s=args.S / t_d,
                       extra_us_per_sample_level=1e6 * (t_d - t_s) / (args.S * L),
                       scalar_spread_us_per_sample_level=1e6 * abs(t_s1 - t_s2) / (args.S * L))
            rows.append(row)
            print(json.dumps(row), flush=True)
        g.ctx().close()
    print("\n| N | L | scalar levels, samples/s (two measurements) | slope levels, samples/s | extra per slope level and "
          "sample (us) | spread of the scalar measurements, same unit (us) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["scalar_samples_per_s"]
        print(f"| {r['n']} | {r['L']} | {a:,.0f} / {b:,.0f} | {r['slope_samples_per_s']:,.0f} | "
              f"{r['extra_us_per_sample_level']:+.2f} | {r['scalar_spread_us_per_sample_level']:.2f} |")


if __name__ == "__main__":
    main()
