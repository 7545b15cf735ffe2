"""Gradient of the outcome log-likelihood (yLogpdfGrad -> gpslc_y_logpdf_grad) against the leave-one-out checks (looPredictive ->
gpslc_y_loo) over the same posterior samples, through the public API.

For N in {1024, 4096} (S = 1024 posterior samples): each call is run once to warm up (workspace, kernel loading), then timed
`--reps` times (best of); every call returns only after its results are on the host, so every timing is device-synchronised.
looPredictive is measured twice, before and after the gradient calls, so that the spread of repeated calls stands next to the
ratio.  Both calls run the Gram build, the factorisation, the back-substitution and W = L^-T; the full gradient adds the pass
over the lower tiles of A^-1 = W W^T (one more factorisation's tile products: three units against two), the call that asks for
dyScale, dyNoise and dY only adds nothing.  The ratio t(gradient) / t(y_loo) is what DESIGN.md §21 records.  Also printed: the
automatic chunk (posterior samples per chunk) of both calls.  That figure is a RESTATEMENT, not read from the library (which does
not report its chunk): carve_chunk's buffers of these two calls and batch_plan.h's 30 % rule, without its 70 % / streams rule and
the fixed 1 MiB — right for one stream on a device nobody else holds memory on, and to be kept in step with carve_chunk by hand.

    python tools/bench_grad.py [--sizes 1024,4096] [--S 1024] [--reps 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_vector_intervention import make_object, timed   # noqa: E402

SCALARS = ("dyScale", "dyNoise", "dY")


def auto_chunk(n, nU, nX, S, total_bytes, grad):
    """samples per chunk of a gpslc_y_loo (grad=False) or full gpslc_y_logpdf_grad call, restated: the per-sample workspace of
    carve_chunk (predict.hip) under 30 % of the device, at most 1048576 / nt^2 (32 .. 16384)"""
    nt = (n + 127) // 128
    Np, tile = nt * 128, 128 * 128
    nlow, tiles_per = nt * (nt + 1) // 2, (nt + 1) * (nt + 2) // 2
    doubles = tiles_per * tile + nt * tile + 2 * Np + 1 + 2 * Np + nlow * tile + Np      # A, inv, sums, z / alpha, W, c
    if grad:
        doubles += nlow * (nU + nX + 1) + nt * nt * nU * 128
    per = 1024 + 8 * doubles
    want = max(32, min(1048576 // (nt * nt), 16384))
    return int(min(want, S, 0.30 * total_bytes // per)), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import causalgpslc_jl_amd as gp
    gp.load_library()
    try:                                   # the device's memory, for the chunk arithmetic only
        import torch
        total = torch.cuda.mem_get_info()[1]
    except Exception:
        total = None
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        g = make_object(gp, n, args.S)
        S = args.S
        ctx = g.ctx()
        call = lambda want: ctx.check(ctx.y_logpdf_grad(S, g.U, None, None, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise,    # noqa: E731
                                                        want=want)[0])
        t1 = timed(lambda: gp.looPredictive(g), args.reps)
        tg = timed(lambda: gp.yLogpdfGrad(g), args.reps)
        ts = timed(lambda: call(SCALARS), args.reps)
        t2 = timed(lambda: gp.looPredictive(g), args.reps)
        row = dict(n=n, S=S, y_loo_s=[t1, t2], grad_s=tg, grad_scalars_only_s=ts, y_loo_samples_per_s=[S / t1, S / t2],
                   grad_samples_per_s=S / tg, ratio=tg / min(t1, t2), ratio_scalars_only=ts / min(t1, t2),
                   chunk_y_loo=total and auto_chunk(n, g.getNU(), g.getNX(), S, total, False)[0],
                   chunk_grad=total and auto_chunk(n, g.getNU(), g.getNX(), S, total, True)[0])
        rows.append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
    print("\n| N | S | y_loo, samples/s (two measurements) | gradient, samples/s | t(gradient) / t(y_loo) | dyScale, dyNoise, dY only | "
          "chunk (restated, see the module text): y_loo / gradient |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["y_loo_samples_per_s"]
        print(f"| {r['n']} | {r['S']} | {a:,.0f} / {b:,.0f} | {r['grad_samples_per_s']:,.0f} | {r['ratio']:.2f} | "
              f"{r['ratio_scalars_only']:.2f} | {r['chunk_y_loo']} / {r['chunk_grad']} |")


if __name__ == "__main__":
    main()
