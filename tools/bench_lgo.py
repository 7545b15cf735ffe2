"""Leave-group-out predictive checks (lgoPredictive -> gpslc_y_lgo) against the leave-one-out checks (looPredictive ->
gpslc_y_loo) over the same posterior samples, through the public API.

For N in {1024, 4096} (S = 1024 posterior samples) and contiguous groups of 16 and of 128 members: each call is run once to
warm up (workspace, kernel loading), then timed `--reps` times (best of); every call returns only after its results are on
the host, so every timing is device-synchronised.  looPredictive is measured twice, before and after the lgoPredictive calls,
so that the spread of repeated calls stands next to the ratios.  Both calls run the same Gram build, factorisation,
back-substitution and W = L^-T; the LOO call then reads W once for the row norms, the LGO call reads it once for the groups'
Gram matrices and factorises them: the ratio t(y_lgo) / t(y_loo) is what DESIGN.md §20 records.  Prints one JSON line per size
and a summary table.

    python tools/bench_lgo.py [--sizes 1024,4096] [--groups 16,128] [--S 1024] [--reps 2]
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
    ap.add_argument("--groups", default="16,128")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    sizes = [int(v) for v in args.groups.split(",")]
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        S = args.S
        t1 = timed(lambda: gp.looPredictive(g), args.reps)
        tg = {m: timed(lambda: gp.lgoPredictive(g, groups=np.arange(n) // m), args.reps) for m in sizes}
        t2 = timed(lambda: gp.looPredictive(g), args.reps)
        row = dict(n=n, S=S, y_loo_s=[t1, t2], y_loo_samples_per_s=[S / t1, S / t2],
                   y_lgo_s={str(m): t for m, t in tg.items()}, y_lgo_samples_per_s={str(m): S / t for m, t in tg.items()},
                   ratio={str(m): t / min(t1, t2) for m, t in tg.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.ctx().close()
    head = " | ".join(f"`y_lgo`, groups of {m}, samples/s | t(`y_lgo`) / t(`y_loo`)" for m in sizes)
    print(f"\n| N | S | `y_loo`, samples/s (two measurements) | {head} |")
    print("|---|---|---|" + "---|---|" * len(sizes))
    for r in rows:
        a, b = r["y_loo_samples_per_s"]
        cells = " | ".join(f"{r['y_lgo_samples_per_s'][str(m)]:,.0f} | {r['ratio'][str(m)]:.2f}" for m in sizes)
        print(f"| {r['n']} | {r['S']} | {a:,.0f} / {b:,.0f} | {cells} |")


if __name__ == "__main__":
    main()
