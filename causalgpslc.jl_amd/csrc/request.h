// A prediction call as an extern "C" entry point receives it (the caller's pointers, host or device, as given), the argument
// checks with the positions of each signature, and the uploads into the ctx's staging pool: what api_predict.hip and
// api_score.hip share on top of predict.h.  The helpers are small and have internal linkage, one copy per entry-point file.
#pragma once
#include "predict.h"

#include <cmath>
#include <cstdio>
#include <initializer_list>

namespace gpslc_host {

// Where a host-pointer prediction over the samples [s0, s0 + S) of S_total sits in the caller's arrays (gpslc_predict_multi:
// one shard; gpslc_predict: s0 = 0, S_total = S).  Per-sample inputs and the outputs are addressed in the caller's FULL
// arrays: element (s, l) of an S_total x L array at (s0 + s) + S_total l, block (s, l) of an n x S_total x L array at
// n ((s0 + s) + S_total l); the level-fastest draw tensor keeps a shard's columns contiguous.
struct HostPlacement {
    int64_t s0 = 0, S_total = 0;
    int64_t ens_off = 0, ens_S = 0;     // Philox stream placement of the shard (ens_S > 0), else the ctx's
};

// what an extern "C" prediction or ITE-distribution function was asked for, with the caller's pointers as given
struct PredictRequest {
    Posterior post;
    Levels lv;
    DrawsAndOutputs out;
    double *MeanITEs = nullptr, *CovITEs = nullptr;     // gpslc_ite_distributions*: S x n, S x n x n
    HostPlacement pl;                                   // host calls
};
static PredictRequest make_request(int64_t S, const SampleParams& samples, int32_t L, const double* doT) {
    PredictRequest rq;
    rq.post.S = S; rq.post.p = samples;
    rq.lv.L = L; rq.lv.doT = doT;
    rq.pl.S_total = S;
    return rq;
}

// The position of each checked argument in one entry point's signature (0: it has no such argument): the k of the status -k
// and of the message's "argument #k".  fp64_only: the entry point refuses a GPSLC_FLAG_FP32_KERNEL context (the fp32 kernel
// mode covers scalar levels without baseline or weights only).
// covW: the joint covariance where the weights are optional (it needs them).
struct ArgPos { int S, U, xyLS, tyLS, L, doT, base, G, W, spp; bool fp64_only; int covW = 0; };
static const ArgPos kPredictArgs{2, 3, 5, 6, 9, 10, 0, 0, 0, 12, false}, kPredictVecArgs{2, 3, 5, 6, 9, 10, 0, 0, 0, 12, true},
    kPredictContrastArgs{2, 3, 5, 6, 9, 10, 11, 0, 0, 13, true}, kPredictWeightedArgs{2, 3, 5, 6, 9, 10, 11, 12, 13, 15, true},
    kPredictMultiArgs{3, 4, 6, 7, 10, 11, 0, 0, 0, 13, false},      // two more leading arguments: nctx, ctxs
    kSamplesArgs{2, 3, 5, 6, 0, 0, 0, 0, 0, 0, false},      // gpslc_ite_distributions, gpslc_y_logpdf, gpslc_y_loo, gpslc_y_lgo, gpslc_likelihood_distribution
    kIteVecArgs{2, 3, 5, 6, 0, 9, 0, 0, 0, 0, true}, kIteContrastArgs{2, 3, 5, 6, 0, 9, 10, 0, 0, 0, true},
    kLikelihoodVecArgs{2, 3, 5, 6, 0, 8, 0, 0, 0, 0, false},
    kPredictSlopeArgs{2, 3, 5, 6, 9, 10, 0, 11, 12, 14, true, 19}, kIteSlopeArgs{2, 3, 5, 6, 0, 9, 0, 0, 0, 0, true};
// the outcome entry points share their twins' positions: gpslc_predict_outcome kPredictSlopeArgs, gpslc_predict_outcome_vec
// kPredictVecArgs, gpslc_ite_distributions_outcome kIteSlopeArgs, gpslc_ite_distributions_outcome_vec kIteVecArgs

// `count` host values: all there and all finite
static int finite_check(gpslc_ctx* c, const double* v, int64_t count, int argk, const char* name) {
    char what[64];
    if (!v) { snprintf(what, sizeof what, "%s is NULL", name); return bad_arg(c, argk, what); }
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) { snprintf(what, sizeof what, "%s has a non-finite entry", name); return bad_arg(c, argk, what); }
    return 0;
}

// The argument checks of every prediction and ITE-distribution entry point, in the order of the arguments.  Levels given as
// host values beyond the plain L scalars (vector levels: n x L; pairs with a baseline; slopes; outcomes; weight columns: n x G) must
// be finite.  The slope and outcome entries take their weights or none (G == 0 and NULL: the plain 1/n average).
static int validate(gpslc_ctx* c, const PredictRequest& rq, const ArgPos& k) {
    const Posterior& po = rq.post;
    const Levels& lv = rq.lv;
    if (!c) return -1;
    if (!c->has_data) { set_err(c, "gpslc_set_data has not been called"); return GPSLC_ERR_NODATA; }
    if (po.S < 0) return bad_arg(c, k.S, "S < 0");
    if (c->nU > 0 && po.S > 0 && (!po.p.U || !po.p.uyLS)) return bad_arg(c, k.U, "U / uyLS must not be NULL when nU > 0");
    if (c->nX > 0 && po.S > 0 && !po.p.xyLS) return bad_arg(c, k.xyLS, "xyLS must not be NULL when nX > 0");
    if (po.S > 0 && (!po.p.tyLS || !po.p.yScale || !po.p.yNoise)) return bad_arg(c, k.tyLS, "tyLS / yScale / yNoise must not be NULL");
    const bool no_spp = rq.out.ite_draws && rq.out.spp < 1;
    int rc = 0;
    if (k.L) {
        if (lv.L < 1) return bad_arg(c, k.L, "L < 1");
        if (!lv.doT) return bad_arg(c, k.doT, "doT is NULL");
        if (no_spp && !k.base && !k.W) return bad_arg(c, k.spp, "spp < 1 with ite_draws requested");      // spp follows doT
        // a placement left over from an earlier, smaller call would make the stream ids (off + s) + S_total * l of this call's
        // last samples collide with the next level's streams: refuse instead of drawing correlated normals
        if (c->ens_S > 0 && c->ens_off + po.S > c->ens_S)
            return bad_arg(c, k.S, "S exceeds the room gpslc_set_ensemble left: sample_offset + S > S_total");
    }
    if (lv.vec || k.base || lv.form == FORM_SLOPE || lv.form == FORM_OUTCOME) {
        if ((rc = finite_check(c, lv.doT, lv.vec ? c->n * (int64_t)lv.L : lv.L, k.doT, "doT"))) return rc;
        // the baselines are optional beside weights
        if (k.base && (lv.base || !k.W) && (rc = finite_check(c, lv.base, lv.L, k.base, "doT_base"))) return rc;
    }
    if (k.W && k.covW) {       // optional weights
        if (lv.G < 0) return bad_arg(c, k.G, "G < 0");
        if (lv.G == 0 && lv.W) return bad_arg(c, k.G, "G == 0 with weights given");
        if (lv.G > 0 && (rc = finite_check(c, lv.W, c->n * (int64_t)lv.G, k.W, "weights"))) return rc;
    } else if (k.W) {
        if (lv.G < 1) return bad_arg(c, k.G, "G < 1");
        if ((rc = finite_check(c, lv.W, c->n * (int64_t)lv.G, k.W, "weights"))) return rc;
    }
    if (no_spp && (k.base || k.W)) return bad_arg(c, k.spp, "spp < 1 with ite_draws requested");
    if (k.covW && rq.out.covW && !lv.W) return bad_arg(c, k.covW, "covW needs weights");
    if (k.fp64_only && (c->flags & GPSLC_FLAG_FP32_KERNEL)) {
        set_err(c, "vector levels, contrasts, slopes, outcomes and weighted effects are not supported on a GPSLC_FLAG_FP32_KERNEL context (fp64 only)");
        return GPSLC_ERR_UNSUPPORTED;
    }
    return 0;
}

// the samples [s0, s0 + S) of a host posterior block, uploaded into the staging pool
static SampleParams upload_samples(gpslc_ctx* c, const SampleParams& h, size_t s0, size_t S) {
    const size_t n = (size_t)c->n, nU = (size_t)c->nU, nX = (size_t)c->nX;
    SampleParams d{};
    d.U = nU ? up(c, h.U + n * nU * s0, n * nU * S) : nullptr;
    d.uyLS = nU ? up(c, h.uyLS + nU * s0, nU * S) : nullptr;
    d.xyLS = nX ? up(c, h.xyLS + nX * s0, nX * S) : nullptr;
    d.tyLS = up(c, h.tyLS + s0, S);
    d.yScale = up(c, h.yScale + s0, S);
    d.yNoise = up(c, h.yNoise + s0, S);
    return d;
}

namespace {

// One output of an outcome-model call: the caller's array (null: not asked), the io's device pointer that stands for it, doubles
struct Output { double* host; double** dev; size_t count; };
using Outputs = std::initializer_list<Output>;
void take_outputs(gpslc_ctx* c, Outputs outs) {            // staging memory for the asked outputs
    for (const Output& o : outs)
        if (o.host) *o.dev = c->io.take<double>(o.count);
}
void deliver_outputs(gpslc_ctx* c, Outputs outs) {
    for (const Output& o : outs)
        if (o.host) copy_out_large(c, o.host, *o.dev, o.count * sizeof(double));
}

}  // namespace

}  // namespace gpslc_host
