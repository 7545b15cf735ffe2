"""Weighted averages over new individuals (averageNew -> gpslc_predict_new_weighted) next to the two routes a user had before:
the mean-only predictNew of the same shape (whose dot product with w gives the mean of the average and no variance) and
predictNew(want_cov=True) followed by the quadratic form w' cov w on the host, through the public API.

For N in {1024, 4096} (S = 256 posterior samples, nX = 4, nU = 1), the outcome form, m in {128, N, 16 N} new individuals and L in
{1, 16} levels: averageNew with G in {1, 8} weight columns, without and with the joint covariance of the levels; predictNew mean
only; and, where the m x m x S x L covariance fits `--cov-gb` (over the first S_cov samples that fit),
predictNew(want_cov=True) plus np.einsum for G = 8 columns.  Each call is run once to warm up (workspace, kernel loading), then
timed `--reps` times (best of); every call returns only after its results are on the host, so every timing is
device-synchronised.  Prints one JSON line per measurement and a summary table (milliseconds per posterior sample).

    python tools/bench_new_average.py [--sizes 1024,4096] [--S 256] [--ms 128,N,16N] [--levels 1,16] [--reps 2] [--cov-gb 8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_new_individuals import first_samples            # noqa: E402
from bench_vector_intervention import make_object, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--ms", default="128,N,16N")
    ap.add_argument("--levels", default="1,16")
    ap.add_argument("--groups", default="1,8")
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
        for L in (int(v) for v in args.levels.split(",")):
            doTs = np.linspace(-1.0, 1.0, L) if L > 1 else np.array([0.4])
            for mtxt in args.ms.split(","):
                m = n * int(mtxt[:-1] or 1) if mtxt.endswith("N") else int(mtxt)
                Xn = rng.standard_normal((m, g.getNX()))
                like = rng.integers(0, n, size=m)
                common = dict(n=n, m=m, L=L)
                record(call="predictNew mean", S=S, G=0, **common,
                       seconds=timed(lambda: gp.predictNew(g, doTs, Xnew=Xn, like=like, want_var=False), args.reps))
                for G in (int(v) for v in args.groups.split(",")):
                    W = rng.random((G, m)) < 0.3         # G random group masks
                    W[:, 0] = True
                    for want_cov in (False, True):
                        record(call="averageNew" + (" + cov" if want_cov else ""), S=S, G=G, **common,
                               seconds=timed(lambda: gp.averageNew(g, doTs, Xnew=Xn, like=like, weights=W, want_cov=want_cov), args.reps))
                s_cov = int(min(S, args.cov_gb * 2.0 ** 30 // (8.0 * m * m * L)))
                if s_cov < 1:
                    print(json.dumps(dict(call="predictNew cov + host w' cov w", skipped="one sample's covariance exceeds --cov-gb",
                                          **common)), flush=True)
                    continue
                if s_cov not in small:
                    small[s_cov] = g if s_cov == S else first_samples(gp, g, s_cov)
                Wf = W / W.sum(axis=1, keepdims=True)

                def dense_route():
                    mean, _, cov = gp.predictNew(small[s_cov], doTs, Xnew=Xn, like=like, want_cov=True)
                    return np.einsum("gi,isl->slg", Wf, mean), np.einsum("gi,slij,gj->slg", Wf, cov, Wf, optimize=True)

                record(call="predictNew cov + host w' cov w", S=s_cov, G=Wf.shape[0], **common, seconds=timed(dense_route, args.reps))
        for o in {id(o): o for o in (g, *small.values())}.values():
            o.ctx().close()
    print("\n| N | m | L | G | call | S | s | ms per sample |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['m']} | {r['L']} | {r['G']} | {r['call']} | {r['S']} | {r['seconds']:.3f} | {r['ms_per_sample']:.3f} |")


if __name__ == "__main__":
    main()
