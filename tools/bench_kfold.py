"""K-fold cross-validation of the outcome model (kfoldPredictive -> gpslc_y_kfold) against the leave-one-out checks
(looPredictive -> gpslc_y_loo) and the leave-group-out checks with groups of 16 (lgoPredictive -> gpslc_y_lgo) over the same
posterior samples, through the public API.

For N in {1024, 4096} (S = 1024 posterior samples) and K = 5 and 10 random folds (foldLabels(N, K, 0): N / K members each, beyond
gpslc_y_lgo's 128 from N = 1024 / K = 5 on): each call is run once to warm up (workspace, kernel loading), then timed `--reps`
times (best of); every call returns only after its results are on the host, so every timing is device-synchronised.
looPredictive is measured twice, before and after the other calls, so that the spread of repeated calls stands next to the
ratios.  All calls run the same Gram build, factorisation, back-substitution and W = L^-T; the K-fold call then builds every
fold's C = W[I, :] W[I, :]^T as tiles (about N^3 / K flops per sample), factorises them (about 2 N^3 / (3 K^2)) and forms
their L^-T for diag(C^-1): by operation count t(y_kfold) / t(y_loo) should be about 1.3 at K = 5 and 1.15 at K = 10 (an
expectation, not a pass mark; DESIGN.md §28 records what was measured).  Prints one JSON line per size and a summary table.

    python tools/bench_kfold.py [--sizes 1024,4096] [--folds 5,10] [--S 1024] [--reps 2]
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
    ap.add_argument("--folds", default="5,10")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    folds = [int(v) for v in args.folds.split(",")]
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        S = args.S
        t1 = timed(lambda: gp.looPredictive(g), args.reps)
        tk = {K: timed(lambda: gp.kfoldPredictive(g, K=K, seed=0), args.reps) for K in folds}
        t16 = timed(lambda: gp.lgoPredictive(g, groups=np.arange(n) // 16), args.reps)
        t2 = timed(lambda: gp.looPredictive(g), args.reps)
        row = dict(n=n, S=S, y_loo_s=[t1, t2], y_loo_samples_per_s=[S / t1, S / t2], y_lgo16_s=t16, y_lgo16_samples_per_s=S / t16,
                   y_kfold_s={str(K): t for K, t in tk.items()}, y_kfold_samples_per_s={str(K): S / t for K, t in tk.items()},
                   ratio={str(K): t / min(t1, t2) for K, t in tk.items()}, ratio_lgo16=t16 / min(t1, t2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.ctx().close()
    head = " | ".join(f"`y_kfold`, K = {K}, samples/s | t(`y_kfold`) / t(`y_loo`)" for K in folds)
    print(f"\n| N | S | `y_loo`, samples/s (two measurements) | `y_lgo`, groups of 16, samples/s | {head} |")
    print("|---|---|---|---|" + "---|---|" * len(folds))
    for r in rows:
        a, b = r["y_loo_samples_per_s"]
        cells = " | ".join(f"{r['y_kfold_samples_per_s'][str(K)]:,.0f} | {r['ratio'][str(K)]:.2f}" for K in folds)
        print(f"| {r['n']} | {r['S']} | {a:,.0f} / {b:,.0f} | {r['y_lgo16_samples_per_s']:,.0f} | {cells} |")


if __name__ == "__main__":
    main()
