"""New individuals at per-individual levels (predictNew with (L, m) levels -> gpslc_predict_new_vec) and the score of a held-out
test set (testPredictive -> gpslc_y_test) next to the calls they are measured against, over the same posterior samples, through
the public API.

For N in {1024, 4096} (S = 256 posterior samples), the outcome form, m in {128, N} new individuals and L in {1, 16} levels: the
vector call (mean only, mean + var, mean + var + cov) and in the same run the scalar predictNew at the same (N, m, L); at m = N
also predict(..., outcome=True, want_mean_ite=True) with an (L, n) vector level, which visits the same N^2 pairs with the same
number of exps per pair and level.  Then testPredictive with a test set of m individuals next to kfoldPredictive(K = N / m) at the
same N.  Each call is run once to warm up, then timed `--reps` times (best of); every call returns only after its results are on
the host, so every timing is device-synchronised.  A covariance is m x m x S x L doubles on the device and on the host: where that
exceeds `--cov-gb` the covariance calls run over the first S_cov samples that fit, and times are reported per sample.
Prints one JSON line per measurement and a summary table (milliseconds per posterior sample).

    python tools/bench_new_vec.py [--sizes 1024,4096] [--S 256] [--reps 2] [--cov-gb 8]
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
from bench_new_individuals import first_samples            # noqa: E402


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
            Dn = doTs[:, None] + 0.3 * rng.standard_normal((L, n))
            record(call="predict outcome at (L, n) levels, MeanITE", n=n, m=n, L=L, S=S,
                   seconds=timed(lambda: gp.predict(g, Dn, want_mean_ite=True, outcome=True), args.reps))
            for mtxt in args.ms.split(","):
                m = n if mtxt == "N" else int(mtxt)
                Xn = rng.standard_normal((m, g.getNX()))
                like = rng.integers(0, n, size=m)
                D = doTs[:, None] + 0.3 * rng.standard_normal((L, m))
                common = dict(n=n, m=m, L=L)
                for name, lv in (("scalar", doTs), ("vector", D)):
                    record(call=f"predictNew {name} mean", S=S, **common,
                           seconds=timed(lambda: gp.predictNew(g, lv, Xnew=Xn, like=like, want_var=False), args.reps))
                    record(call=f"predictNew {name} mean + var", S=S, **common,
                           seconds=timed(lambda: gp.predictNew(g, lv, Xnew=Xn, like=like), args.reps))
                s_cov = fewer(m, L)
                if s_cov < 1:
                    print(json.dumps(dict(call="predictNew mean + var + cov", skipped="one sample's covariance exceeds --cov-gb",
                                          **common)), flush=True)
                    continue
                for name, lv in (("scalar", doTs), ("vector", D)):
                    record(call=f"predictNew {name} mean + var + cov", S=s_cov, **common,
                           seconds=timed(lambda: gp.predictNew(small[s_cov], lv, Xnew=Xn, like=like, want_cov=True), args.reps))
        for mtxt in args.ms.split(","):
            m = n if mtxt == "N" else int(mtxt)
            Xt, like = rng.standard_normal((m, g.getNX())), rng.integers(0, n, size=m)
            Tt, Yt = rng.standard_normal(m), rng.standard_normal(m)
            record(call="testPredictive", n=n, m=m, L=1, S=S,
                   seconds=timed(lambda: gp.testPredictive(g, Xt, Tt, Yt, like=like), args.reps))
            record(call=f"kfoldPredictive K = {max(n // m, 1)}", n=n, m=m, L=1, S=S,
                   seconds=timed(lambda: gp.kfoldPredictive(g, K=max(n // m, 1)), args.reps))
        for o in {id(o): o for o in (g, *small.values())}.values():
            o.ctx().close()
    print("\n| N | m | L | call | S | s | ms per sample |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['m']} | {r['L']} | {r['call']} | {r['S']} | {r['seconds']:.3f} | {r['ms_per_sample']:.3f} |")


if __name__ == "__main__":
    main()
