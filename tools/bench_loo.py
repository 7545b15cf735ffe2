"""Leave-one-out predictive checks (looPredictive -> gpslc_y_loo) against the marginal likelihood (yLogpdf -> gpslc_y_logpdf)
over the same posterior samples, through the public API.

For N in {1024, 4096} (S = 1024 posterior samples): each call is run once to warm up (workspace, kernel loading), then timed
`--reps` times (best of); both return only after their results are on the host, so every timing is device-synchronised.
yLogpdf is measured twice, before and after looPredictive, so that the spread of repeated calls stands next to the ratio.  The
LOO call runs the same Gram build and factorisation, then the back-substitution, W = L^-T (about one more factorisation's
products) and the row norms: the ratio t(y_loo) / t(y_logpdf) is what DESIGN.md §18 records.  Prints one JSON line per size
and a summary table.

    python tools/bench_loo.py [--sizes 1024,4096] [--S 1024] [--reps 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_vector_intervention import make_object, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        S = args.S
        t1 = timed(lambda: gp.yLogpdf(g), args.reps)
        tl = timed(lambda: gp.looPredictive(g), args.reps)
        t2 = timed(lambda: gp.yLogpdf(g), args.reps)
        row = dict(n=n, S=S, y_logpdf_s=[t1, t2], y_loo_s=tl, y_logpdf_samples_per_s=[S / t1, S / t2],
                   y_loo_samples_per_s=S / tl, ratio=tl / min(t1, t2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.ctx().close()
    print("\n| N | S | y_logpdf, samples/s (two measurements) | y_loo, samples/s | t(y_loo) / t(y_logpdf) |")
    print("|---|---|---|---|---|")
    for r in rows:
        a, b = r["y_logpdf_samples_per_s"]
        print(f"| {r['n']} | {r['S']} | {a:,.0f} / {b:,.0f} | {r['y_loo_samples_per_s']:,.0f} | {r['ratio']:.2f} |")


if __name__ == "__main__":
    main()
