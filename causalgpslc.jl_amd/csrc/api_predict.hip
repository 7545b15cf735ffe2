// Entry points of include/gpslc_hip.h that describe a prediction call: gpslc_predict* and gpslc_predict_multi,
// gpslc_ite_distributions*, gpslc_predict_new*, gpslc_y_test, gpslc_likelihood_distribution*.
#include "request.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

extern "C" {

// device pointers everywhere; the info words come from the staging pool (the caller has reset it)
static int predict_dev_inner(gpslc_ctx* c, const PredictRequest& rq) {
    PredictIO io;
    io.post = rq.post; io.lv = rq.lv; io.out = rq.out; io.X = c->dX;
    io.MeanITEs = rq.MeanITEs; io.CovITEs = rq.CovITEs;
    io.ens_off = rq.pl.ens_off; io.ens_S = rq.pl.ens_S;
    io.info = c->io.take<int>((size_t)rq.post.S);
    run_predict(c, io);
    return first_info(c);
}

int gpslc_predict_dev(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                      const double* tyLS, const double* yScale, const double* yNoise, int32_t L,
                      const double* doT, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                      double* meanSATE, double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictArgs);
    if (rc) return rc;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        c->io.reset();
        return predict_dev_inner(c, rq);
    });
}

// The body of the host-pointer entry points (an empty call returns here, after its checks): uploads, run_predict, delivery —
// every level's run of a shard goes from the device straight to its place in the caller's array (no host staging, VERDICT r05
// item 2)
static int predict_host(gpslc_ctx* c, const PredictRequest& rq) {
    const int64_t S = rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const Levels& lv = rq.lv;
        const DrawsAndOutputs& o = rq.out;
        const size_t n = (size_t)c->n, L = (size_t)lv.L;
        const size_t LR = lv.W ? L * lv.G : L;     // meanSATE / varSATE columns: levels, or levels x weight columns
        const size_t s0 = (size_t)rq.pl.s0, St = (size_t)rq.pl.S_total;
        c->io.reset();
        PredictRequest d = rq;             // the same request with device pointers
        d.post.p = upload_samples(c, rq.post.p, s0, (size_t)S);
        d.lv.doT = up(c, lv.doT, lv.vec ? n * L : L);                 // vector levels: n x L
        d.lv.base = lv.base ? up(c, lv.base, L) : nullptr;            // contrasts: the L baselines
        if (lv.W) {                // n x G host (weights[i + n*g]) -> column fastest on the device (W[g + G*i]: the kernels' layout)
            const size_t G = (size_t)lv.G;
            std::vector<double> wt(n * G);
            for (size_t i = 0; i < n; ++i)
                for (size_t g = 0; g < G; ++g) wt[g + G * i] = lv.W[i + n * g];
            d.lv.W = up(c, wt.data(), wt.size());
        }
        d.out.z = nullptr;
        if (o.z && o.ite_draws) {  // caller's normals n x spp x S_total x L: level l of the shard is one run of n spp S doubles
            double* dz = c->io.take<double>(n * o.spp * S * L);
            const size_t run = n * o.spp * (size_t)S * sizeof(double);
            HC(hipMemcpy2D(dz, run, o.z + n * o.spp * s0, n * o.spp * St * sizeof(double), run, L, hipMemcpyHostToDevice));
            d.out.z = dz;
        }
        double* oms = d.out.meanSATE = o.meanSATE ? c->io.take<double>((size_t)S * LR) : nullptr;
        // the joint covariance takes its diagonal from the device's varW, asked for or not
        double* ovs = d.out.varSATE = (o.varSATE || o.covW) ? c->io.take<double>((size_t)S * LR) : nullptr;
        double* ocv = d.out.covW = o.covW ? c->io.take<double>((size_t)S * LR * L) : nullptr;
        double* omi = d.out.meanITE = o.meanITE ? c->io.take<double>(n * S * L) : nullptr;
        double* odr = d.out.ite_draws = o.ite_draws ? c->io.take<double>(L * n * S * o.spp) : nullptr;
        int st = predict_dev_inner(c, d);
        if (st < 0) return st;
        const size_t sb = (size_t)S * sizeof(double);
        if (o.meanSATE) HC(hipMemcpy2D(o.meanSATE + s0, St * sizeof(double), oms, sb, sb, LR, hipMemcpyDeviceToHost));
        if (o.varSATE) HC(hipMemcpy2D(o.varSATE + s0, St * sizeof(double), ovs, sb, sb, LR, hipMemcpyDeviceToHost));
        if (o.covW) copy_out_rows(c, o.covW + s0, St * sizeof(double), ocv, sb, LR * L);
        if (o.meanITE) copy_out_rows(c, o.meanITE + n * s0, n * St * sizeof(double), omi, n * sb, L);
        // level-fastest tensor L x n x (S_total spp): a sample's columns are one contiguous run
        if (o.ite_draws) copy_out_large(c, o.ite_draws + L * n * o.spp * s0, odr, sizeof(double) * L * n * S * o.spp);
        return st;
    });
}

int gpslc_predict(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                  const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                  double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                  double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictArgs);
    return rc ? rc : predict_host(c, rq);
}

// vector levels: every entry of the n x L host array doT must be finite
int gpslc_predict_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                      const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                      double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                      double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.vec = true;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictVecArgs);
    return rc ? rc : predict_host(c, rq);
}

// contrasts: level l is the pair (doT[l], doT_base[l]) of finite scalars
int gpslc_predict_contrast(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                           const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                           const double* doT_base, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                           double* meanSATE, double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictContrastArgs);
    return rc ? rc : predict_host(c, rq);
}

// weighted effects: G >= 1 columns of n finite host weights each; scalar levels, with or without baselines
int gpslc_predict_weighted(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                           const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                           const double* doT_base, int32_t G, const double* weights, double pred_noise, int32_t spp,
                           uint64_t seed, const double* z, double* meanW, double* varW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base); rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictWeightedArgs);
    return rc ? rc : predict_host(c, rq);
}

// the same call with the joint covariance of the levels per weight column as one more output
int gpslc_predict_curve(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                        const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                        const double* doT_base, int32_t G, const double* weights, double pred_noise, int32_t spp,
                        uint64_t seed, const double* z, double* meanW, double* varW, double* covW, double* meanITE,
                        double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base); rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictWeightedArgs);
    return rc ? rc : predict_host(c, rq);
}

// marginal effects: level l is the slope d f_i(t) / dt at the finite scalar t = doT[l].  G == 0 and NULL weights:
// the plain 1/n average as gpslc_predict's (covW must be NULL); else G >= 1 weight columns as gpslc_predict_curve's
int gpslc_predict_slope(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                        const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                        int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                        double* meanW, double* varW, double* covW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.form = FORM_SLOPE; rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictSlopeArgs);
    return rc ? rc : predict_host(c, rq);
}

// potential outcomes: level l is f_i(doT[l]) itself, everybody set to the finite scalar doT[l].  Arguments, weights
// (or none) and checks are gpslc_predict_slope's
int gpslc_predict_outcome(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                          const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                          int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                          double* meanW, double* varW, double* covW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.form = FORM_OUTCOME; rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictSlopeArgs);
    return rc ? rc : predict_host(c, rq);
}

// the outcome at vector levels: individual i set to doT[i + n*l]; arguments and checks are gpslc_predict_vec's
int gpslc_predict_outcome_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                              const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                              double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                              double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.vec = true; rq.lv.form = FORM_OUTCOME;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictVecArgs);
    return rc ? rc : predict_host(c, rq);
}

// The sharded ensemble behind the ABI (the loop src/prediction.jl:30-33 over src/estimation.jl:78-84): contiguous
// blocks of the posterior-sample index over the contexts, one host thread per context, data replicated (every ctx holds its own
// copy: gpslc_set_data), no traffic between the devices while they compute.  The "gather" is each device's own device-to-host
// copy into ITS block of the caller's arrays — nctx PCIe links in parallel, nothing funnels through one GPU — and since round 6
// every level's run of a shard goes from the device (through the ctx's pinned bounce chunks) straight to its place in the
// caller's array: no per-shard host staging, no second pass over the results.  A shard's ensemble placement travels as a
// parameter: the contexts' own gpslc_set_ensemble state is read (ctxs[0]'s places the whole call), never written.
int gpslc_predict_multi(int32_t nctx, gpslc_ctx* const* ctxs, int64_t S, const double* U, const double* uyLS,
                        const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise, int32_t L,
                        const double* doT, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                        double* meanSATE, double* varSATE, double* meanITE, double* ite_draws, int32_t* info_or_null) {
    if (nctx < 1) return -1;
    if (!ctxs) return -2;
    for (int k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return -2;
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return bad_arg(ctxs[0], 2, "the same ctx is listed twice (one ctx per shard: calls on a ctx are serialised)");
    }
    gpslc_ctx* c0 = ctxs[0];
    for (int k = 1; k < nctx; ++k) {
        if (ctxs[k]->n != c0->n || ctxs[k]->nX != c0->nX || ctxs[k]->nU != c0->nU)
            return bad_arg(c0, 2, "the contexts differ in n / nX / nU");
        // one precision mode per call: a ctx created with GPSLC_FLAG_FP32_KERNEL would silently mix arithmetics across the shards
        if ((ctxs[k]->flags & GPSLC_FLAG_FP32_KERNEL) != (c0->flags & GPSLC_FLAG_FP32_KERNEL))
            return bad_arg(c0, 2, "the contexts differ in GPSLC_FLAG_FP32_KERNEL");
        if (!ctxs[k]->has_data) { set_err(c0, "gpslc_set_data has not been called on every ctx"); return GPSLC_ERR_NODATA; }
    }
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc0 = validate(c0, rq, kPredictMultiArgs);      // argument numbers of THIS signature, in the code and in the message
    if (rc0) return rc0;
    if (S == 0) { for (int k = 0; k < nctx; ++k) ctxs[k]->last_info.clear(); return GPSLC_OK; }
    try {
        // placement of the whole call (ctxs[0]'s, if the caller set one: this call may itself be one node's share)
        const int64_t base_off = c0->ens_S > 0 ? c0->ens_off : 0, total = c0->ens_S > 0 ? c0->ens_S : S;
        struct Shard { int64_t s0 = 0, Sr = 0; int rc = 0; };
        std::vector<Shard> sh((size_t)nctx);
        for (int k = 0; k < nctx; ++k) {
            int64_t s1 = 0;
            (void)gpslc_shard_range(S, nctx, k, &sh[(size_t)k].s0, &s1);
            sh[(size_t)k].Sr = s1 - sh[(size_t)k].s0;
        }
        auto work = [&](int k) {
            Shard& h = sh[(size_t)k];
            if (h.Sr == 0) { ctxs[k]->last_info.clear(); return; }
            PredictRequest part = rq;                // the shard's samples, placed in the caller's full arrays
            part.post.S = h.Sr;
            part.pl = HostPlacement{h.s0, S, base_off + h.s0, total};
            h.rc = predict_host(ctxs[k], part);
        };
        std::vector<std::thread> pool;
        for (int k = 1; k < nctx; ++k) {
            try { pool.emplace_back(work, k); }
            catch (...) { work(k); }                 // no thread to be had: this shard runs here, in turn
        }
        work(0);
        for (auto& t : pool) t.join();
        int rc = 0;
        for (int k = 0; k < nctx && rc == 0; ++k)
            if (sh[(size_t)k].rc < 0) {
                rc = sh[(size_t)k].rc;
                if (k > 0) set_err(c0, "shard " + std::to_string(k) + " (device " + std::to_string(ctxs[k]->device) + "): " + ctxs[k]->err);
            }
        for (int k = 0; k < nctx && rc == 0; ++k) rc = sh[(size_t)k].rc;        // blocks are in sample order: the first failing pivot
        if (info_or_null)
            for (int k = 0; k < nctx; ++k) {
                const Shard& h = sh[(size_t)k];
                if (h.Sr == 0) continue;
                if ((int64_t)ctxs[k]->last_info.size() == h.Sr) memcpy(info_or_null + h.s0, ctxs[k]->last_info.data(), sizeof(int32_t) * h.Sr);
                else for (int64_t j = 0; j < h.Sr; ++j) info_or_null[h.s0 + j] = 0;
            }
        return rc;
    } catch (const std::bad_alloc&) {
        set_err(c0, "host allocation failed");
        return GPSLC_ERR_NOMEM;
    } catch (...) {
        set_err(c0, "internal error");
        return GPSLC_ERR_INTERNAL;
    }
}

// gpslc_ite_distributions*'s body: one level (host) — a scalar, n values (vec), the contrast of two scalars (base), a slope or
// an outcome (scalar or vec)
static int ite_distributions_host(gpslc_ctx* c, const PredictRequest& rq) {
    const int64_t S = rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t n = (size_t)c->n;
        c->io.reset();
        PredictRequest d = rq;             // the same request with device pointers
        d.post.p = upload_samples(c, rq.post.p, 0, (size_t)S);
        d.lv.doT = up(c, rq.lv.doT, rq.lv.vec ? n : 1);
        d.lv.base = rq.lv.base ? up(c, rq.lv.base, 1) : nullptr;
        d.MeanITEs = rq.MeanITEs ? c->io.take<double>((size_t)S * n) : nullptr;
        d.CovITEs = rq.CovITEs ? c->io.take<double>((size_t)S * n * n) : nullptr;
        const int st = predict_dev_inner(c, d);
        if (rq.MeanITEs) HC(hipMemcpy(rq.MeanITEs, d.MeanITEs, sizeof(double) * S * n, hipMemcpyDeviceToHost));
        if (rq.CovITEs) copy_out_large(c, rq.CovITEs, d.CovITEs, sizeof(double) * (size_t)S * n * n);
        return st;
    });
}

int gpslc_ite_distributions(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                            const double* tyLS, const double* yScale, const double* yNoise, double doT,
                            double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kSamplesArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                const double* tyLS, const double* yScale, const double* yNoise, const double* doT,
                                double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, doT);
    rq.lv.vec = true;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteVecArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_contrast(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                     const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                     double doT_base, double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.against(&doT_base);
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteContrastArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_slope(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                  const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                  double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.form = FORM_SLOPE;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteSlopeArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_outcome(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                    const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                    double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.form = FORM_OUTCOME;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteSlopeArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_outcome_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                        const double* tyLS, const double* yScale, const double* yNoise, const double* doT,
                                        double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, doT);
    rq.lv.vec = true; rq.lv.form = FORM_OUTCOME;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteVecArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

// The checks gpslc_predict_new and gpslc_predict_new_weighted share: the samples, then arguments 9 - 15 (m, Xnew, Unew, form, L,
// doT, doT_base), which sit at the same positions in both
// the samples and the new individuals themselves (arguments 2 - 11 of every call that takes new individuals)
static int validate_new_rows(gpslc_ctx* c, const PredictRequest& rq, const ArgPos& k, int64_t m, const double* Xnew, const double* Unew) {
    const int64_t S = rq.post.S;
    int rc = validate(c, rq, k);
    if (rc) return rc;
    if (m < 1 || m > (int64_t)GP_TS * 32767) return bad_arg(c, 9, "m < 1 (or beyond 32767 row tiles)");
    if ((c->nX > 0) != (Xnew != nullptr)) return bad_arg(c, 10, c->nX > 0 ? "Xnew is NULL but nX > 0" : "Xnew given but nX == 0");
    if (Xnew && (rc = finite_check(c, Xnew, m * c->nX, 10, "Xnew"))) return rc;
    if ((c->nU > 0) != (Unew != nullptr)) return bad_arg(c, 11, c->nU > 0 ? "Unew is NULL but nU > 0" : "Unew given but nU == 0");
    if (Unew && (rc = finite_check(c, Unew, m * c->nU * S, 11, "Unew"))) return rc;
    return 0;
}
// vec (gpslc_predict_new_vec): doT and doT_base are m x L, and the slope is no form of the call
static int validate_new(gpslc_ctx* c, const PredictRequest& rq, int64_t m, const double* Xnew, const double* Unew, int32_t form,
                        const double* doT_base, bool vec = false) {
    static const ArgPos kNewArgs{2, 3, 5, 6, 13, 14, 0, 0, 0, 0, true};
    const int32_t L = rq.lv.L;
    const double* doT = rq.lv.doT;
    int rc = validate_new_rows(c, rq, kNewArgs, m, Xnew, Unew);
    if (rc) return rc;
    if (form != GPSLC_NEW_OUTCOME && form != GPSLC_NEW_CONTRAST && form != GPSLC_NEW_SLOPE)
        return bad_arg(c, 12, "unknown form (GPSLC_NEW_OUTCOME, GPSLC_NEW_CONTRAST or GPSLC_NEW_SLOPE: the ordinary effect f(a) - f(T) "
                              "needs a factual treatment, which a new individual does not have)");
    if (vec && form == GPSLC_NEW_SLOPE)
        return bad_arg(c, 12, "unsupported form: the slope at per-individual levels is not offered (GPSLC_NEW_OUTCOME or GPSLC_NEW_CONTRAST)");
    const int64_t nlev = vec ? m * L : L;
    if ((rc = finite_check(c, doT, nlev, 14, "doT"))) return rc;
    if (form == GPSLC_NEW_CONTRAST) {
        if ((rc = finite_check(c, doT_base, nlev, 15, "doT_base"))) return rc;
    } else if (doT_base) {
        return bad_arg(c, 15, "doT_base given for a form that is no contrast");
    }
    return 0;
}
// ... and their uploads: the samples, the levels of the form and the new individuals' features
static PredictIO new_io(gpslc_ctx* c, const PredictRequest& rq, int64_t m, const double* Xnew, const double* Unew, int32_t form,
                        const double* doT_base, double pred_noise, bool vec = false) {
    const size_t mm = (size_t)m, S = (size_t)rq.post.S, L = (size_t)rq.lv.L * (vec ? (size_t)m : 1);
    PredictIO io;
    io.post.S = rq.post.S; io.post.p = upload_samples(c, rq.post.p, 0, S);
    io.X = c->dX;
    io.lv.L = rq.lv.L; io.lv.doT = up(c, rq.lv.doT, L);
    io.lv.form = form == GPSLC_NEW_OUTCOME ? FORM_OUTCOME : form == GPSLC_NEW_SLOPE ? FORM_SLOPE : FORM_CONTRAST;
    io.lv.base = doT_base ? up(c, doT_base, L) : nullptr;
    io.out.pred_noise = pred_noise;
    io.fresh.m = (int)m; io.fresh.vec = vec;
    io.fresh.Xnew = Xnew ? up(c, Xnew, mm * c->nX) : nullptr;
    io.fresh.Unew = Unew ? up(c, Unew, mm * c->nU * S) : nullptr;
    return io;
}

// predictions for m new individuals (vec: at per-individual levels, §29): host pointers; every check before any
// device work
static int predict_new_host(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                            const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                            int32_t form, int32_t L, const double* doT, const double* doT_base, double pred_noise, double* mean,
                            double* var, double* cov, bool vec) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    int rc = validate_new(c, rq, m, Xnew, Unew, form, doT_base, vec);
    if (rc) return rc;
    if (!std::isfinite(pred_noise)) return bad_arg(c, 16, "pred_noise is not finite");
    if (!mean && !var && !cov) return bad_arg(c, 17, "mean, var and cov are all NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t mm = (size_t)m, SL = (size_t)S * L;
        c->io.reset();
        PredictIO io = new_io(c, rq, m, Xnew, Unew, form, doT_base, pred_noise, vec);
        const Outputs outs = {{mean, &io.fresh.mean, mm * SL}, {var, &io.fresh.var, mm * SL}, {cov, &io.fresh.cov, mm * mm * SL}};
        take_outputs(c, outs);
        if (cov && !var) io.fresh.var = c->io.take<double>(mm * SL);      // the covariance takes its diagonal from it
        io.info = c->io.take<int>((size_t)S);
        run_predict(c, io);
        const int st = first_info(c);
        deliver_outputs(c, outs);
        if (st > 0)      // a sample whose factorisation broke down: NaN in everything of it
            for (int64_t s = 0; s < S; ++s) {
                if (c->last_info[(size_t)s] == 0) continue;
                for (int64_t l = 0; l < L; ++l) {
                    const size_t o = mm * (size_t)(s + S * l);
                    if (mean) std::fill(mean + o, mean + o + mm, NAN);
                    if (var) std::fill(var + o, var + o + mm, NAN);
                    if (cov) std::fill(cov + mm * o, cov + mm * (o + mm), NAN);
                }
            }
        return st;
    });
}

int gpslc_predict_new(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                      const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                      int32_t form, int32_t L, const double* doT, const double* doT_base, double pred_noise, double* mean,
                      double* var, double* cov) {
    return predict_new_host(c, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, form, L, doT, doT_base, pred_noise, mean, var,
                            cov, false);
}

// ... at per-individual levels: doT and doT_base are m x L
int gpslc_predict_new_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                          const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                          int32_t form, int32_t L, const double* doT, const double* doT_base, double pred_noise, double* mean,
                          double* var, double* cov) {
    return predict_new_host(c, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, form, L, doT, doT_base, pred_noise, mean, var,
                            cov, true);
}

// The score of a held-out test set: the outcome form at the test set's own treatments with the observation's
// noise, the pointwise log densities and the joint one.  Arguments 9 - 11 and their checks are gpslc_predict_new's.
int gpslc_y_test(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                 const double* yScale, const double* yNoise, int64_t m, const double* Xtest, const double* Utest,
                 const double* Ttest, const double* Ytest, double* mean, double* var, double* lpd, double* lpd_joint) {
    static const ArgPos kTestArgs{2, 3, 5, 6, 0, 0, 0, 0, 0, 0, true};
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, Ttest);
    int rc = validate_new_rows(c, rq, kTestArgs, m, Xtest, Utest);
    if (rc) return rc;
    if ((rc = finite_check(c, Ttest, m, 12, "Ttest"))) return rc;
    if ((rc = finite_check(c, Ytest, m, 13, "Ytest"))) return rc;
    if (!mean && !var && !lpd && !lpd_joint) return bad_arg(c, 14, "mean, var, lpd and lpd_joint are all NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t mm = (size_t)m, mS = mm * (size_t)S;
        c->io.reset();
        PredictIO io = new_io(c, rq, m, Xtest, Utest, GPSLC_NEW_OUTCOME, nullptr, 0.0, true);
        io.fresh.Ytest = up(c, Ytest, mm);
        const Outputs outs = {{mean, &io.fresh.mean, mS}, {var, &io.fresh.var, mS}, {lpd, &io.fresh.lpd, mS},
                              {lpd_joint, &io.fresh.lpd_joint, (size_t)S}};
        take_outputs(c, outs);
        if (!mean) io.fresh.mean = c->io.take<double>(mS);      // the densities read both
        if (!var) io.fresh.var = c->io.take<double>(mS);
        io.info = c->io.take<int>((size_t)S);
        run_predict(c, io);
        const int st = first_info(c);
        deliver_outputs(c, outs);
        if (st > 0)      // a sample whose factorisation of A broke down: NaN in everything of it
            for (int64_t s = 0; s < S; ++s) {
                if (c->last_info[(size_t)s] == 0) continue;
                for (double* o : {mean, var, lpd})
                    if (o) std::fill(o + mm * (size_t)s, o + mm * (size_t)(s + 1), NAN);
                if (lpd_joint) lpd_joint[s] = NAN;
            }
        return st;
    });
}

// weighted averages over m new individuals: gpslc_predict_new's checks, then G >= 1 columns of m finite weights
int gpslc_predict_new_weighted(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                               const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                               int32_t form, int32_t L, const double* doT, const double* doT_base, int32_t G, const double* weights,
                               double pred_noise, double* meanW, double* varW, double* covW) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    int rc = validate_new(c, rq, m, Xnew, Unew, form, doT_base);
    if (rc) return rc;
    if (G < 1) return bad_arg(c, 16, "G < 1");
    if ((rc = finite_check(c, weights, m * (int64_t)G, 17, "weights"))) return rc;
    if (!std::isfinite(pred_noise)) return bad_arg(c, 18, "pred_noise is not finite");
    if (!meanW && !varW && !covW) return bad_arg(c, 19, "meanW, varW and covW are all NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t mm = (size_t)m, Gs = (size_t)G, SR = (size_t)S * L * Gs;
        c->io.reset();
        PredictIO io = new_io(c, rq, m, Xnew, Unew, form, doT_base, pred_noise);
        io.fresh.weighted = true;
        {       // m x G host (weights[i + m*g]) -> column fastest on the device (W[g + G*i]), as predict_host does
            std::vector<double> wt(mm * Gs);
            for (size_t i = 0; i < mm; ++i)
                for (size_t g = 0; g < Gs; ++g) wt[g + Gs * i] = weights[i + mm * g];
            io.lv.W = up(c, wt.data(), wt.size());
            io.lv.G = G;
        }
        const Outputs outs = {{meanW, &io.out.meanSATE, SR}, {varW, &io.out.varSATE, SR}, {covW, &io.out.covW, SR * L}};
        take_outputs(c, outs);
        if (covW && !varW) io.out.varSATE = c->io.take<double>(SR);      // the joint covariance takes its diagonal from it
        io.info = c->io.take<int>((size_t)S);
        run_predict(c, io);
        const int st = first_info(c);
        deliver_outputs(c, outs);
        if (st > 0)      // a sample whose factorisation broke down: NaN in everything of it (sample fastest in every output)
            for (const Output& o : outs)
                for (size_t s = 0; o.host && s < (size_t)S; ++s)
                    if (c->last_info[s] != 0)
                        for (size_t k = s; k < o.count; k += (size_t)S) o.host[k] = NAN;
        return st;
    });
}

// doTv: null = the scalar doT, else the per-individual intervention (n, host)
static int likelihood_distribution_impl(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                        double tyLS, double yScale, double yNoise, double doT, const double* doTv,
                                        double* CovWW, double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                        double* CovC21, double* CovC22) {
    const double ty = tyLS, ysc = yScale, yno = yNoise;
    return guarded(c, [&]() {
        ensure_streams(c);
        StreamSlot& slot = c->slots[0];
        hipStream_t st = slot.st;
        const int n = (int)c->n, nt = c->nt;
        const long long nlow = (long long)nt * (nt + 1) / 2, nsq = (long long)nt * nt;
        DevBuffer<double> bdo, tiles, inv, rect, outb;
        DevBuffer<int> info;
        c->io.reset();
        SampleParams sp = upload_samples(c, SampleParams{U, uyLS, xyLS, &ty, &ysc, &yno}, 0, 1);
        sp.u_sstride = (long long)n * c->nU;
        info.reserve(sizeof(int));
        HC(hipMemsetAsync(info, 0, sizeof(int), st));
        tiles.reserve((size_t)nlow * GP_TSQ * 8);
        inv.reserve((size_t)nt * GP_TSQ * 8);
        rect.reserve((size_t)6 * nsq * GP_TSQ * 8);      // K, Ks, Ks', Kss, W1, W2
        outb.reserve((size_t)n * n * 8);
        double* rb = rect;
        const long long rs = nsq * GP_TSQ;
        TRef Kt = rect_ref(rb, rs, nt), Kst = rect_ref(rb + rs, rs, nt), KsTt = rect_ref(rb + 2 * rs, rs, nt),
             Ksst = rect_ref(rb + 3 * rs, rs, nt), W1 = rect_ref(rb + 4 * rs, rs, nt), W2 = rect_ref(rb + 5 * rs, rs, nt);
        TRef M = lower_ref(tiles, nlow * GP_TSQ);
        // A = K + yNoise I (lower tiles) and its factor
        const SampleGrid grid{c->dX, c->dT, sp, 0, n, c->nX, c->nU, nt};
        GramArgs ga{grid};
        ga.M = M; ga.part = nullptr; ga.with_sums = 0; ga.f32 = 0;
        launch_gram(ga, 1, st);
        factor_panels(c, slot, M, nt, nt, inv, info, 0, 1, 0, false, 0);
        LdBuildArgs la{grid, doT, Kt, Kst, KsTt, Ksst};
        if (doTv) la.doTv = up(bdo, doTv, (size_t)n);
        launch_ld_build(la, st);
        auto emit = [&](const TRef& R, double* host, double diag_add) {
            if (!host) return;
            launch_rect_gather(RectGatherArgs{R, n, nt, outb, diag_add}, st);
            HC(hipStreamSynchronize(st));
            copy_out_large(c, host, outb, (size_t)n * n * 8);
        };
        emit(Kt, CovWW, 0.0);
        emit(Kst, CovWWs, 0.0);
        emit(Kt, CovWWp, yno);
        if (CovC11 || CovC12 || CovC21 || CovC22) {
            // W1 = K L^-T, W2 = Ks' L^-T  (copies, then unit B's tile-level left-looking solve)
            HC(hipMemcpyAsync(W1.base, Kt.base, (size_t)rs * 8, hipMemcpyDeviceToDevice, st));
            HC(hipMemcpyAsync(W2.base, KsTt.base, (size_t)rs * 8, hipMemcpyDeviceToDevice, st));
            TRef invref = inv_ref(inv, nt);
            w_solve(c, slot, W1, M, invref, nt, 1, nt);
            w_solve(c, slot, W2, M, invref, nt, 1, nt);
            // C11 = K - W1 W1', C12 = Ks - W1 W2', C21 = Ks' - W2 W1', C22 = Kss - W2 W2'   (src/likelihood.jl:46-49)
            auto block = [&](const TRef& Cm, const TRef& Wa, const TRef& Wb, double* host) {
                if (!host) return;
                gemm(c, tile_rect(Wa, Wb, Cm, 0, 0, nt, nt, 0, nt, 1), slot, 0);
                emit(Cm, host, 0.0);
            };
            block(Kt, W1, W1, CovC11);      // K, Ks, Ks', Kss are consumed in place: emitted above already
            block(Kst, W1, W2, CovC12);
            block(KsTt, W2, W1, CovC21);
            block(Ksst, W2, W2, CovC22);
        }
        HC(hipStreamSynchronize(st));
        HC(hipGetLastError());
        int hinfo = 0;
        HC(hipMemcpy(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost));
        c->last_info.assign(1, hinfo);
        return hinfo;
    });
}

int gpslc_likelihood_distribution(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                  double tyLS, double yScale, double yNoise, double doT, double* CovWW,
                                  double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                  double* CovC21, double* CovC22) {
    int rc = validate(c, make_request(1, {U, uyLS, xyLS, &tyLS, &yScale, &yNoise}, 0, nullptr), kSamplesArgs);
    if (rc) return rc;
    return likelihood_distribution_impl(c, U, uyLS, xyLS, tyLS, yScale, yNoise, doT, nullptr, CovWW, CovWWs, CovWWp, CovC11,
                                        CovC12, CovC21, CovC22);
}

int gpslc_likelihood_distribution_vec(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                      double tyLS, double yScale, double yNoise, const double* doT, double* CovWW,
                                      double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                      double* CovC21, double* CovC22) {
    PredictRequest rq = make_request(1, {U, uyLS, xyLS, &tyLS, &yScale, &yNoise}, 1, doT);
    rq.lv.vec = true;
    int rc = validate(c, rq, kLikelihoodVecArgs);
    if (rc) return rc;
    return likelihood_distribution_impl(c, U, uyLS, xyLS, tyLS, yScale, yNoise, 0.0, doT, CovWW, CovWWs, CovWWp, CovC11,
                                        CovC12, CovC21, CovC22);
}

}  // extern "C"
