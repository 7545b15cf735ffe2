"""Scalar against per-individual (vector) intervention levels through the public API (causalgpslc_jl_amd.predict).

For N in {1024, 4096} (S = 1024 posterior samples) and L in {1, 4, 16} levels: every shape is run once to warm up (workspace,
kernel loading), then timed `--reps` times (best of); predict() returns only after the results are on the host, so every
timing is device-synchronised.  Prints one JSON line per shape and a summary: samples/s, and the extra cost of a vector level
per (sample, level) over a scalar one.

    python tools/bench_vector_intervention.py [--sizes 1024,4096] [--levels 1,4,16] [--S 1024] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_object(gp, n, S, nX=4, nU=1, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, nX))
    T = rng.standard_normal(n)
    Y = np.sin(T) + 0.5 * X[:, 0] + 0.3 * rng.standard_normal(n)
    U = np.asfortranarray(rng.standard_normal((n, nU, S)))
    ig = lambda *shape: np.maximum(4.0 / rng.gamma(4.0, 1.0, size=shape), 0.25)   # noqa: E731
    return gp.GPSLCObject(X, T, Y, U, ig(nU, S), ig(nX, S), ig(S), ig(S), ig(S))


def timed(fn, reps):
    fn()                                   # warm-up
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--levels", default="1,4,16")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        rng = np.random.default_rng(n)
        for L in (int(v) for v in args.levels.split(",")):
            xs = np.linspace(-0.5, 0.5, L)
            # vector levels: everyone shifted, or half the individuals left as observed
            D = np.stack([np.where(rng.random(n) < 0.5, g.T, g.T + x) if l % 2 else g.T + x for l, x in enumerate(xs)])
            t_s = timed(lambda: gp.predict(g, xs, want_mean_ite=True), args.reps)
            t_v = timed(lambda: gp.predict(g, D, want_mean_ite=True), args.reps)
            row = dict(n=n, S=args.S, L=L, scalar_s=t_s, vector_s=t_v, scalar_samples_per_s=args.S / t_s,
                       vector_samples_per_s=args.S / t_v, extra_us_per_sample_level=1e6 * (t_v - t_s) / (args.S * L),
                       scalar_us_per_sample=1e6 * t_s / args.S)
            rows.append(row)
            print(json.dumps(row), flush=True)
        g.ctx().close()
    print("\n| N | L | scalar samples/s | vector samples/s | extra per vector level and sample (us) |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['L']} | {r['scalar_samples_per_s']:.0f} | {r['vector_samples_per_s']:.0f} | "
              f"{r['extra_us_per_sample_level']:.1f} |")


if __name__ == "__main__":
    main()
