"""Predictions for new individuals (predictNew -> gpslc_predict_new) next to the calls that evaluate the same estimand at the
training individuals, over the same posterior samples, through the public API.

For N in {1024, 4096} (S = 256 posterior samples), the outcome form, m in {128, N} new individuals and L in {1, 16} levels:
mean only, mean + var, and mean + var + cov; and at the same N in the same run predict(..., outcome=True, want_mean_ite=True)
(its MeanITE pass evaluates the N^2 pairs the mean-only call evaluates at m = N) and, where L = 1, ITEDistributions(...,
outcome=True) (its covariance is the m = N covariance).  Each call is run once to warm up (workspace, kernel loading), then timed
`--reps` times (best of); every call returns only after its results are on the host, so every timing is device-synchronised.
A covariance is m x m x S x L doubles on the device and on the host: where that exceeds `--cov-gb` the covariance calls (and
ITEDistributions) run over the first S_cov samples that fit, and their times are reported per sample like all the others.
Prints one JSON line per measurement and a summary table (milliseconds per posterior sample).

    python tools/bench_new_individuals.py [--sizes 1024,4096] [--S 256] [--reps 2] [--cov-gb 8]
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


def first_samples(gp, g, S):
    """the same model over its first S posterior samples"""
    return gp.GPSLCObject(g.X, g.T, g.Y, g.U[:, :, :S], g.uyLS[:, :S], g.xyLS[:, :S], g.tyLS[:S], g.yNoise[:S], g.yScale[:S])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--ms", default="128,N")
    ap.add_argument("--levels", default="1,16")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cov-gb", type=float, default=8.0)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    rows = []

    def record(**row):
        row["ms_per_sample"] = 1e3 * row["seconds"] / row["S"]
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n in (int(v) for v in args.sizes.split(",")):
        S = args.S
        g = make_object(gp, n, S)
        rng = np.random.default_rng(n)
        small = {}                       # the model over fewer samples, for covariances that would not fit

        def fewer(m, L):
            s_cov = int(min(S, args.cov_gb * 2.0 ** 30 // (8.0 * m * m * L)))
            if s_cov >= 1 and s_cov not in small:
                small[s_cov] = g if s_cov == S else first_samples(gp, g, s_cov)
            return s_cov

        for L in (int(v) for v in args.levels.split(",")):
            doTs = np.linspace(-1.0, 1.0, L) if L > 1 else np.array([0.4])
            record(call="predict outcome, MeanITE", n=n, m=n, L=L, S=S,
                   seconds=timed(lambda: gp.predict(g, doTs, want_mean_ite=True, outcome=True), args.reps))
            if L == 1:
                s_cov = fewer(n, 1)
                if s_cov >= 1:
                    record(call="ITEDistributions outcome", n=n, m=n, L=1, S=s_cov,
                           seconds=timed(lambda: gp.ITEDistributions(small[s_cov], 0.4, outcome=True), args.reps))
            for mtxt in args.ms.split(","):
                m = n if mtxt == "N" else int(mtxt)
                Xn = rng.standard_normal((m, g.getNX()))
                like = rng.integers(0, n, size=m)
                common = dict(n=n, m=m, L=L)
                record(call="predictNew mean", S=S, **common,
                       seconds=timed(lambda: gp.predictNew(g, doTs, Xnew=Xn, like=like, want_var=False), args.reps))
                record(call="predictNew mean + var", S=S, **common,
                       seconds=timed(lambda: gp.predictNew(g, doTs, Xnew=Xn, like=like), args.reps))
                s_cov = fewer(m, L)
                if s_cov < 1:
                    print(json.dumps(dict(call="predictNew mean + var + cov", skipped="one sample's covariance exceeds --cov-gb",
                                          **common)), flush=True)
                    continue
                record(call="predictNew mean + var + cov", S=s_cov, **common,
                       seconds=timed(lambda: gp.predictNew(small[s_cov], doTs, Xnew=Xn, like=like, want_cov=True), args.reps))
        for o in {id(o): o for o in (g, *small.values())}.values():
            o.ctx().close()
    print("\n| N | m | L | call | S | s | ms per sample |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['m']} | {r['L']} | {r['call']} | {r['S']} | {r['seconds']:.3f} | {r['ms_per_sample']:.3f} |")


if __name__ == "__main__":
    main()
