// Entry points of include/gpslc_hip.h that score: the outcome model (gpslc_y_logpdf, gpslc_y_loo, gpslc_y_lgo, gpslc_y_kfold,
// gpslc_y_logpdf_grad), the Gaussian-process nodes (gpslc_gp_logpdf, gpslc_nodes_*) and the dense-covariance nodes with their
// cache (gpslc_mvn_*); the single-workgroup node path and the switch between it and the tiled score.
#include "request.h"
#include "sm_layout.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

namespace {

// ---- single-launch small-n node scores ----------------------------------------------------------------------------
struct HostNode {            // host view of one node (gpslc_node with plain pointers)
    int nF;
    const double* F[2];      // up to two column groups + one extra column are concatenated into the feature block:
    int nFpart[2];           //   F[0] (nFpart[0] columns), F[1] (nFpart[1] columns), then `col` (one column) if non-null
    const double* col;
    const double* ls[2];     // lengthscales of the two groups; ls_col for the extra column
    double ls_col;
    double scale, noise;
    const double* target;
    const double* dev_cov;   // dense-covariance node: n x n in device memory (else null), and its scale factor
    double covscale;
};

// The three kinds of node view.  An RBF node: K = scale exp(-sum_f ((x_if - x_jf) / ls_f)^2) + noise I over nF feature columns
HostNode rbf_node(int nF, const double* F, const double* ls, double scale, double noise, const double* target) {
    HostNode h{};
    h.nF = nF; h.F[0] = nF ? F : nullptr; h.nFpart[0] = nF; h.ls[0] = nF ? ls : nullptr;
    h.scale = scale; h.noise = noise; h.target = target;
    return h;
}
// the :Y node: the same over the feature parts U | X | T (T one column with the scalar lengthscale tyLS)
HostNode y_node(int nU, const double* U, const double* uyLS, int nX, const double* X, const double* xyLS, const double* T,
                double tyLS, double scale, double noise, const double* target) {
    HostNode h = rbf_node(nU, U, uyLS, scale, noise, target);
    h.nF = nU + nX + 1;
    h.F[1] = nX ? X : nullptr; h.nFpart[1] = nX; h.ls[1] = nX ? xyLS : nullptr;
    h.col = T; h.ls_col = tyLS;
    return h;
}
// a dense-covariance node: K = covscale dev_cov (n x n, device)
HostNode dense_node(const double* dev_cov, double covscale, const double* target) {
    HostNode h{};
    h.dev_cov = dev_cov; h.covscale = covscale; h.target = target;
    return h;
}

// log N(x; 0, K) of an n-vector from log det K and the quadratic form x' K^-1 x
constexpr double kLog2Pi = 1.8378770664093454835606594728112;
inline double gauss_logpdf(size_t n, double logdet, double quad) { return -0.5 * ((double)n * kLog2Pi + logdet + quad); }

// A node score can run as ONE workgroup of one launch: matrix resident in LDS (n <= 160..176), or the left-looking
// kernel with the finished block columns in an L2-resident scratch (n <= 640).  The latter keeps one CU busy per node
// for 100+ us: worth it up to a few hundred nodes per call, beyond that the batched tiled path wins.
bool fast_path_ok(const gpslc_ctx* c, int nF_max, int64_t count) {
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) return false;
    if (small_gp_lds_bytes((int)c->n, nF_max) <= kLdsCapBytes) return count <= 4096;
    return MidLayout::fits((int)c->n) && count <= 512;
}

// The gradient outputs of gpslc_nodes_logpdf_grad (host, any may be null): dF and dls are the nodes' n x nF_i blocks and nF_i
// values concatenated in node order, dscale and dnoise hold `count` values, dtarget is n x count
struct NodeGradOut {
    double *dF, *dls, *dscale, *dnoise, *dtarget;
    bool any() const { return dF || dls || dscale || dnoise || dtarget; }
};

// scores `count` nodes in ONE launch; logdet/quad/info per node come back through the pinned buffer.
// Returns the first failing pivot (0 = all fine); logpdf[i] = gauss_logpdf(n, logdet_i, quad_i).
// draw_out (optional, host, n x count): node i also returns chol(K_i) * target_i.
// grad (optional; RBF nodes that fit small_grad_lds_bytes): the same launch also differentiates every score (k_small.hip); a
// node whose factorisation broke down gets NaN.
int small_nodes_logpdf(gpslc_ctx* c, int count, const HostNode* nodes, double* logpdf, double* draw_out = nullptr,
                       const NodeGradOut* grad = nullptr) {
    ensure_streams(c);
    const size_t n = (size_t)c->n;
    auto stage = [&](int i) { return NodeStage(n, (size_t)nodes[i].nF, grad != nullptr); };     // sm_layout.h
    size_t doubles = 0, gdoubles = 0;
    int nF_max = 0;
    for (int i = 0; i < count; ++i) {
        doubles += stage(i).in_total; gdoubles += stage(i).out_total;
        nF_max = std::max(nF_max, nodes[i].nF);
    }
    const size_t off_out = ((size_t)count * sizeof(SmallNode) + 63) & ~size_t(63);
    const size_t off_data = off_out + NodeStage::header((size_t)count) * sizeof(double);
    const size_t off_draw = off_data + doubles * sizeof(double);          // [count][n] draws (pinned, written by the kernel)
    const size_t off_grad = off_draw + (draw_out ? (size_t)count * n * sizeof(double) : 0);     // the gradient launch's result block
    c->pin.reserve((off_grad + gdoubles * sizeof(double) + 4095) & ~size_t(4095));
    void* dbase = nullptr;
    HC(hipHostGetDevicePointer(&dbase, c->pin, 0));
    char* dev = static_cast<char*>(dbase);
    SmallNode* hn = c->pin.as<SmallNode>();
    double* hout = reinterpret_cast<double*>(c->pin + off_out);
    double* hd = reinterpret_cast<double*>(c->pin + off_data);
    double* dd = reinterpret_cast<double*>(dev + off_data);
    size_t o = 0, go = 0;        // where node i's input and results start
    for (int i = 0; i < count; ++i) {
        const HostNode& h = nodes[i];
        const NodeStage S = stage(i);
        SmallNode& sn = hn[i];
        sn.nF = h.nF; sn.gofs = (int)go; sn.scale = h.scale; sn.noise = h.noise;
        sn.cov = h.dev_cov; sn.covscale = h.covscale;
        sn.Fs = dd + o;
        sn.target = dd + o + S.target;
        // a feature column goes in twice: divided by its lengthscale, x * (1 / l), the arithmetic of the general path, and
        // (gradient) as it is with the lengthscale, because D comes from the raw features
        size_t f = 0;
        auto put = [&](const double* col, double l) {
            const double il = 1.0 / l;
            for (size_t r = 0; r < n; ++r) hd[o + f * n + r] = col[r] * il;
            if (grad) { memcpy(hd + o + S.raw + f * n, col, n * sizeof(double)); hd[o + S.ls + f] = l; }
            ++f;
        };
        for (int g = 0; g < 2; ++g)
            for (int k = 0; k < h.nFpart[g]; ++k) put(h.F[g] + (size_t)k * n, h.ls[g][k]);
        if (h.col) put(h.col, h.ls_col);
        memcpy(hd + o + S.target, h.target, n * sizeof(double));
        o += S.in_total; go += S.out_total;
    }
    SmallArgs a{};
    a.nodes = reinterpret_cast<const SmallNode*>(dev);
    for (int i = 0; i < std::min(count, SMALL_INLINE_NODES); ++i) a.inl[i] = hn[i];
    a.n = (int)n; a.NB = (int)((n + 15) / 16);
    a.out = reinterpret_cast<double*>(dev + off_out);
    a.draw = draw_out ? reinterpret_cast<double*>(dev + off_draw) : nullptr;
    const bool in_lds = grad || small_gp_lds_bytes((int)n, nF_max) <= kLdsCapBytes;
    if (grad && small_grad_lds_bytes((int)n, nF_max) > kLdsCapBytes) throw std::runtime_error("gradient launch beyond its LDS image");
    if (!in_lds) {       // mid-size kernel: per-node scratch for the finished block columns and the scaled features
        const size_t per = (mid_gp_scratch_doubles((int)n, nF_max) + 31) & ~size_t(31);
        c->scratch.reserve(per * (size_t)count * sizeof(double) + 256);
        c->scratch.reset();
        a.scratch = c->scratch.take<double>(per * (size_t)count);
        a.scratch_stride = (long long)per;
    }
#ifdef GPSLC_DIAG
    static const int want_stamps = diag_env("GPSLC_SMALL_STAMPS", 0);
    if (want_stamps) a.stamps = a.out + NodeStage::kResult * (size_t)count;
#endif
    hipStream_t st = c->slots[0].st;
    if (grad) launch_small_grad(a, reinterpret_cast<double*>(dev + off_grad), count, nF_max, st);
    else if (in_lds) launch_small_gp(a, count, nF_max, st);
    else launch_mid_gp(a, count, nF_max, st);
    HC(hipGetLastError());
    HC(hipStreamSynchronize(st));
#ifdef GPSLC_DIAG
    if (want_stamps && in_lds) {
        static int printed = 0;
        const double* sp = hout + NodeStage::kResult * (size_t)count;
        if (printed++ < want_stamps)
            fprintf(stderr, "small_gp stamps (shader clocks): inputs %.0f gram %.0f factor+panel %.0f (wave 0 inside the pivot chains: %.0f) update %.0f total %.0f\n",
                    sp[0], sp[1], sp[2], sp[4], sp[3], sp[5]);
    }
    if (want_stamps && !in_lds) {      // node 0, per wave: cumulative shader clocks of the phases over all block columns
        static int printed = 0;
        const double* sp = hout + (NodeStage::kResult + NodeStage::kStamps) * (size_t)count;
        if (printed++ < want_stamps)
            for (int w = 0; w < kSmWaves; ++w, sp += NodeStage::kWaveStamps / kSmWaves)
                fprintf(stderr, "mid_gp wave %d: gram %.0f k-loop %.0f to-LDS %.0f wait %.0f factor+store %.0f wait %.0f\n", w,
                        sp[0], sp[1], sp[2], sp[3], sp[4], sp[5]);
    }
#endif
    if (draw_out) memcpy(draw_out, c->pin + off_draw, (size_t)count * n * sizeof(double));
    int first = 0;
    c->last_info.resize((size_t)count);
    for (int i = 0; i < count; ++i) {
        const double* res = hout + NodeStage::kResult * (size_t)i;        // logdet, quad, info
        const int info = (int)res[2];
        c->last_info[i] = info;
        if (info != 0 && first == 0) first = info;
        logpdf[i] = gauss_logpdf(n, res[0], res[1]);
    }
    if (grad) {
        const double* r = reinterpret_cast<const double*>(c->pin + off_grad);
        size_t fo = 0, lo = 0;        // node i's slots of dF and dls
        auto deliver = [](double* dst, const double* src, size_t cnt, bool bad) {
            if (!dst) return;
            if (bad) std::fill(dst, dst + cnt, (double)NAN);
            else memcpy(dst, src, cnt * sizeof(double));
        };
        for (int i = 0; i < count; ++i) {
            const NodeStage S = stage(i);
            const size_t nF = (size_t)nodes[i].nF;
            const bool bad = c->last_info[i] != 0;
            deliver(grad->dF ? grad->dF + fo : nullptr, r, n * nF, bad);
            deliver(grad->dls ? grad->dls + lo : nullptr, r + S.dls, nF, bad);
            deliver(grad->dscale ? grad->dscale + i : nullptr, r + S.dscale, 1, bad);
            deliver(grad->dnoise ? grad->dnoise + i : nullptr, r + S.dnoise, 1, bad);
            deliver(grad->dtarget ? grad->dtarget + (size_t)i * n : nullptr, r + S.dtarget, n, bad);
            fo += n * nF; lo += nF; r += S.out_total;
        }
    }
    return first;
}

// ---- node scores: the six entry points of the chain's inner loop and what they share --------------------------------
// The tiled score of the S parameter sets of `io`: the caller has filled in the samples, the features, the right-hand side
// (the value being scored) and, for gpslc_nodes_draw, the node draw.  This adds "no level, score only", runs the prediction
// pass and turns the epilogue's logdet / quad into log-densities.  Returns the first failing pivot.
int tiled_score(gpslc_ctx* c, PredictIO& io, double* logpdf) {
    const size_t S = (size_t)io.post.S;
    const double zero = 0.0;
    io.lv.L = 0; io.lv.doT = up(c, &zero, 1);
    io.logdet = c->io.take<double>(S); io.quad = c->io.take<double>(S); io.info = c->io.take<int>(S);
    run_predict(c, io);
    std::vector<double> ld(S), q(S);
    HC(hipMemcpy(ld.data(), io.logdet, sizeof(double) * S, hipMemcpyDeviceToHost));
    HC(hipMemcpy(q.data(), io.quad, sizeof(double) * S, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; ++s) logpdf[s] = gauss_logpdf((size_t)c->n, ld[s], q[s]);
    return first_info(c);
}

// The body of the outcome-model entry points that score on the tiled factor (gpslc_y_logpdf beyond the single-workgroup kernels,
// gpslc_y_loo, gpslc_y_lgo, gpslc_y_logpdf_grad), after their checks: uploads the request's samples and the
// overrides (Y_or_null: the value being scored — Gen passes it to logpdf — else the ctx's Y), lets `special` add what only this
// call has, takes device memory for the asked outputs (`outs` points into io) and scores.  Nothing is copied out after a negative status.
int outcome_call(gpslc_ctx* c, const PredictRequest& rq, const double* X_or_null, const double* Y_or_null, double* logpdf_or_null,
                 PredictIO& io, Outputs outs, const std::function<void()>& special = nullptr) {
    const size_t n = (size_t)c->n, S = (size_t)rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        c->io.reset();
        io.post.S = rq.post.S; io.post.p = upload_samples(c, rq.post.p, 0, S);
        io.X = (X_or_null && c->nX) ? up(c, X_or_null, n * c->nX) : c->dX;
        if (Y_or_null) { io.Y = up(c, Y_or_null, n); io.y_sstride = 0; }
        if (special) special();
        take_outputs(c, outs);
        std::vector<double> lp(logpdf_or_null ? 0 : S);       // the scores are computed either way: kept only when the caller asks
        const int st = tiled_score(c, io, logpdf_or_null ? logpdf_or_null : lp.data());
        if (st >= 0) deliver_outputs(c, outs);
        return st;
    });
}

// general (tiled, multi-launch) path of gpslc_gp_logpdf; arguments already validated
// draws_or_null (host, n x S; needs t_shared == 0): also chol(K_s) target_s — the targets are then standard normals
// grad_or_null (host, the layouts of S sets of nF columns: dF n x nF x S, dls nF x S, dtarget n x S): also the gradient of every
// score, §21's pair pass and finish kernel in node mode (GradArgs::no_t)
int gp_logpdf_general(gpslc_ctx* c, int64_t S, int32_t nF, const double* F, int32_t f_shared, const double* ls,
                      const double* scale, const double* noise, const double* target, int32_t t_shared, double* logpdf,
                      double* draws_or_null = nullptr, const NodeGradOut* grad_or_null = nullptr) {
    const size_t n = (size_t)c->n;
    c->io.reset();
    const double* dF = nF ? up(c, F, n * nF * (f_shared ? 1 : S)) : nullptr;
    const double* dls = nF ? up(c, ls, (size_t)nF * S) : nullptr;
    const double* dsc = up(c, scale, S);
    const double* dno = up(c, noise, S);
    const double* dtg = up(c, target, n * (t_shared ? 1 : S));
    std::vector<double> inf(S, INFINITY);        // tyLS = inf switches the treatment term off: e_ij = exp(-0) = 1
    const double* dty = up(c, inf.data(), S);
    PredictIO io;
    io.post.S = S;
    io.post.p = SampleParams{dF, dls, nullptr, dty, dsc, dno, f_shared ? 0 : (long long)n * nF};
    io.p_shared_u = f_shared != 0;
    io.X = nullptr; io.nU = nF; io.nX = 0;
    io.Y = dtg; io.y_sstride = t_shared ? 0 : (long long)n;
    double* ddraw = nullptr;
    if (draws_or_null) {
        ensure_streams(c);
        ddraw = c->io.take<double>(n * (size_t)S);
        double* zero_mean = c->io.take<double>(n * (size_t)S);
        HC(hipMemsetAsync(zero_mean, 0, n * (size_t)S * sizeof(double), c->slots[0].st));
        HC(hipStreamSynchronize(c->slots[0].st));
        io.nz = dtg; io.nzero = zero_mean; io.ndraw = ddraw;
    }
    NodeGradOut g = grad_or_null ? *grad_or_null : NodeGradOut{};
    if (nF == 0) g.dF = g.dls = nullptr;
    const Outputs outs = {{g.dF, &io.grad.U, n * (size_t)nF * S}, {g.dls, &io.grad.uyLS, (size_t)nF * S}, {g.dscale, &io.grad.yScale, (size_t)S},
                          {g.dnoise, &io.grad.yNoise, (size_t)S}, {g.dtarget, &io.grad.Y, n * (size_t)S}};
    io.grad_no_t = true;
    take_outputs(c, outs);
    const int st = tiled_score(c, io, logpdf);
    if (draws_or_null) HC(hipMemcpy(draws_or_null, ddraw, n * (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    deliver_outputs(c, outs);
    return st;
}

// ONE batched pass of the general tiled path over all nodes of a call (S = count parameter sets with per-set feature blocks
// and per-set targets); draws_or_null: also chol(K_i) target_i per node (gpslc_nodes_draw)
int nodes_general(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, int nF_max, double* logpdf, double* draws_or_null,
                  const NodeGradOut* grad_or_null = nullptr) {
    // Nodes with fewer than nF_max feature columns are padded with zero
    // columns of lengthscale 1: a padding column adds (0 * 1 - 0 * 1)^2 = +0.0 to every squared distance, so a
    // node's Gram matrix — and its score — is bit-identical to the one its own feature count would give.
    // Staging lives in the ctx (this call sits in the MCMC inner loop: no allocation once the buffers have grown),
    // and nodes that all share ONE feature block — the nX `:X => k => :X` nodes, F = U for every k — hand it over once
    // (f_shared) instead of count padded copies.
    const size_t n = (size_t)c->n;
    bool same_f = true;
    for (int i = 1; i < count; ++i) same_f = same_f && nodes[i].F == nodes[0].F && nodes[i].nF == nodes[0].nF;
    std::vector<double>& Fp = c->stage_f;
    std::vector<double>& rest = c->stage_rest;       // [ls | scale | noise | targets]
    const size_t ls_n = (size_t)std::max(nF_max, 1) * count;
    rest.resize(ls_n + 2 * (size_t)count + n * (size_t)count);
    double* lsp = rest.data();
    double* sc = lsp + ls_n;
    double* no = sc + count;
    double* tg = no + count;
    std::fill(lsp, lsp + ls_n, 1.0);
    if (!same_f) {
        Fp.resize(n * (size_t)nF_max * count);
        std::fill(Fp.begin(), Fp.end(), 0.0);
    }
    for (int i = 0; i < count; ++i) {
        const gpslc_node& q = nodes[i];
        if (q.nF > 0) {
            if (!same_f) memcpy(Fp.data() + (size_t)i * n * nF_max, q.F, n * (size_t)q.nF * sizeof(double));
            memcpy(lsp + (size_t)i * nF_max, q.ls, (size_t)q.nF * sizeof(double));
        }
        sc[i] = q.scale; no[i] = q.noise;
        memcpy(tg + (size_t)i * n, q.target, n * sizeof(double));
    }
    const double* Fsrc = nF_max == 0 ? nullptr : (same_f ? nodes[0].F : Fp.data());
    if (!grad_or_null)
        return gp_logpdf_general(c, count, nF_max, Fsrc, same_f ? 1 : 0, nF_max ? lsp : nullptr, sc, no, tg, 0, logpdf, draws_or_null);
    // The gradient comes back in the padded layout (count sets of nF_max columns, one block per node even where the nodes share
    // their features); the padding columns' gradients are dropped here.  A real column's sums do not see the padding: K adds
    // +0.0 per padding column and every feature is summed on its own, so a node's bits do not depend on the widest node.
    const NodeGradOut& g = *grad_or_null;
    std::vector<double> pF(g.dF ? n * (size_t)nF_max * count : 0), pls(g.dls ? (size_t)nF_max * count : 0);
    const NodeGradOut padded{g.dF ? pF.data() : nullptr, g.dls ? pls.data() : nullptr, g.dscale, g.dnoise, g.dtarget};
    const int st = gp_logpdf_general(c, count, nF_max, Fsrc, same_f ? 1 : 0, nF_max ? lsp : nullptr, sc, no, tg, 0, logpdf, nullptr, &padded);
    size_t fo = 0, lo = 0;
    for (int i = 0; i < count && st >= 0; ++i) {
        const size_t nF = (size_t)nodes[i].nF;
        if (g.dF && nF) memcpy(g.dF + fo, pF.data() + (size_t)i * n * nF_max, n * nF * sizeof(double));
        if (g.dls && nF) memcpy(g.dls + lo, pls.data() + (size_t)i * nF_max, nF * sizeof(double));
        fo += n * nF; lo += nF;
    }
    return st;
}

// The argument checks of the fused node calls (`out`: the output the call must deliver, argument 4 of both signatures):
// the largest feature count of the nodes, or the negative status
int nodes_check(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, const double* out, const char* out_is_null) {
    if (!c) return -1;
    if (count < 0) return bad_arg(c, 2, "count < 0");
    if (count > 0 && !nodes) return bad_arg(c, 3, "nodes is NULL");
    if (count > 0 && !out) return bad_arg(c, 4, out_is_null);
    int nF_max = 0;
    for (int i = 0; i < count; ++i) {
        const gpslc_node& q = nodes[i];
        if (q.nF < 0 || q.nF > 32 || (q.nF > 0 && (!q.F || !q.ls)) || !q.target)
            return bad_arg(c, 3, "node with nF outside 0..32 or a NULL feature / lengthscale / target pointer");
        nF_max = std::max(nF_max, (int)q.nF);
    }
    return nF_max;
}

// The body of the fused node calls: every node one workgroup of ONE launch, or — beyond the single-workgroup kernels (n > 640,
// many nodes, fp32 kernel mode) — the batched tiled factorisation of every node's covariance; with draws_or_null also
// chol(K_i) target_i per node (the small kernels' draw mode; L z on the predictive-draw kernel, round 6)
int nodes_score(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, int nF_max, double* logpdf_or_null, double* draws_or_null) {
    if (count == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        std::vector<double> lp;                      // the scores are computed either way: kept only when the caller asks
        if (!logpdf_or_null) { lp.resize((size_t)count); logpdf_or_null = lp.data(); }
        if (!fast_path_ok(c, nF_max, count)) return nodes_general(c, count, nodes, nF_max, logpdf_or_null, draws_or_null);
        std::vector<HostNode> hn;
        hn.reserve((size_t)count);
        for (int i = 0; i < count; ++i) {
            const gpslc_node& q = nodes[i];
            hn.push_back(rbf_node(q.nF, q.F, q.ls, q.scale, q.noise, q.target));
        }
        return small_nodes_logpdf(c, count, hn.data(), logpdf_or_null, draws_or_null);
    });
}

// both paths of gpslc_mvn_logpdf / gpslc_mvn_draw can run on this ctx (n <= 640): then the dense covariance is always kept
bool mvn_dual(const gpslc_ctx* c) { return fast_path_ok(c, 0, 1); }

// the tiled factor of the device covariance dcov (substitution-based: SigmaU * uNoise is near-singular by construction, 1e-13
// jitter, src/utils.jl:17-33); mvn.logdet / mvn.info from it, and it now stands for hand-over mvn.gen
void mvn_factor_tiles(gpslc_ctx* c, const double* dcov) {
    ensure_streams(c);
    const int nt = c->nt;
    const long long nlow = (long long)nt * (nt + 1) / 2;
    StreamSlot& slot = c->slots[0];
    hipStream_t st = slot.st;
    c->mvn.tiles_gen = 0;
    c->mvn.tiles.reserve((size_t)nlow * GP_TSQ * 8);
    DevBuffer<double> old, oq;
    DevBuffer<int> info;
    old.reserve(8); oq.reserve(8); info.reserve(sizeof(int));
    HC(hipMemsetAsync(info, 0, sizeof(int), st));
    TRef M = lower_ref(c->mvn.tiles, nlow * GP_TSQ);
    launch_dense_load(DenseLoadArgs{dcov, (int)c->n, nt, M}, st);
    factor_robust(c, slot, M, nt, info, 0, 1, 0);
    launch_quad_rows(QuadRowsArgs{M, (int)c->n, nt, 0, 0, old, oq}, st);
    HC(hipStreamSynchronize(st));
    HC(hipGetLastError());
    HC(hipMemcpy(&c->mvn.logdet, old, 8, hipMemcpyDeviceToHost));
    HC(hipMemcpy(&c->mvn.info, info, sizeof(int), hipMemcpyDeviceToHost));
    c->mvn.tiles_gen = c->mvn.gen;
}

// the tiled solve of gpslc_mvn_logpdf against the cached factor: z_s = L^-1 x_s for all S vectors (host, n x S) as the rows of
// W = X^T L^-T, a tile-level solve; returns |z_s|^2 (device, S values in the ctx's staging pool), the stream drained
const double* mvn_solve_tiles(gpslc_ctx* c, int64_t S, const double* x) {
    ensure_streams(c);
    const int n = (int)c->n, nt = c->nt;
    const long long nlow = (long long)nt * (nt + 1) / 2;
    StreamSlot& slot = c->slots[0];
    hipStream_t st = slot.st;
    const int naug = (int)((S + GP_TS - 1) / GP_TS);
    c->io.reset();
    const double* dx = up(c, x, (size_t)n * S);
    double* wt = c->io.take<double>((size_t)naug * nt * GP_TSQ);
    double* oq = c->io.take<double>((size_t)S);
    TRef W = rect_ref(wt, (long long)naug * nt * GP_TSQ, nt);
    TRef Ls = lower_ref(c->mvn.tiles, nlow * GP_TSQ);
    launch_rows_rhs(RowsRhsArgs{dx, S, n, nt, naug, W, 0, 1}, st);
    const int short_rows = naug == 1 ? (int)S : 0;
    // right-looking: z_k = w_k L_kk^-T by substitution (no inverted block: the factor is near-singular), then every
    // remaining column block in parallel on the MFMA tile kernel
    for (int k = 0; k < nt; ++k) {
        launch_trsm_robust(W, Ls, k, 0, naug, 1, st);
        if (k + 1 < nt)     // W(:, j) -= W(:, k) L(j, k)^T for j > k
            gemm(c, short_aug_row(tile_rect(W, Ls, W, 0, k + 1, naug, nt - k - 1, k, k + 1, 1), 0, short_rows), slot, 0);
    }
    launch_row_norms(RowNormArgs{W, nt, naug, S, oq}, st);
    HC(hipStreamSynchronize(st));
    HC(hipGetLastError());
    return oq;
}

// hands a covariance over: n <= 640 keeps the dense matrix (and validates it on the single-workgroup kernel when the call takes
// that path), the tiled path factorises it; mvn.info = its LAPACK-style info
void mvn_cache(gpslc_ctx* c, const double* cov, bool small) {
    const size_t n = (size_t)c->n;
    c->mvn.valid = false;
    ++c->mvn.gen;
    if (!mvn_dual(c)) {      // n > 640 (or the fp32 kernel mode): the tiled path is the only one
        DevBuffer<double> bcov;
        mvn_factor_tiles(c, up(bcov, cov, n * n));
        c->mvn.valid = true;
        return;
    }
    c->mvn.dense.reserve(n * n * sizeof(double));
    HC(hipMemcpy(c->mvn.dense, cov, n * n * sizeof(double), hipMemcpyHostToDevice));
    if (small) {
        // validate once (as the tiled path does when it factorises): info of cov itself
        std::vector<double> zeros(n, 0.0);
        const HostNode probe = dense_node(c->mvn.dense, 1.0, zeros.data());
        double dummy = 0.0;
        c->mvn.info = small_nodes_logpdf(c, 1, &probe, &dummy);
    } else {
        mvn_factor_tiles(c, c->mvn.dense);
    }
    c->mvn.valid = true;
}

// before a cov = NULL call on the tiled path: the factor of the latest hand-over (rebuilt from the dense copy when an earlier
// hand-over went to the single-workgroup path)
void mvn_tiles_current(gpslc_ctx* c) {
    if (c->mvn.tiles && c->mvn.tiles_gen == c->mvn.gen) return;
    mvn_factor_tiles(c, c->mvn.dense);
}

// What gpslc_mvn_logpdf and gpslc_mvn_draw do before they differ (`in`: x / z, argument 5; `out`: the result, argument 6):
// the pointer checks, then — small: the call runs on the single-workgroup kernels — the covariance is handed over, or the tiled
// factor brought up to date when the call runs tiled and gave none, and every vector's info is that of the covariance.
// `body(small)` goes on from there; mvn.info != 0 and S == 0 are its to answer (the two calls differ there).
template <class Body>
int mvn_call(gpslc_ctx* c, int64_t S, const double* cov, const double* in, const char* in_is_null, const double* out,
             const char* out_is_null, Body&& body) {
    if (!c) return -1;
    if (S < 0) return bad_arg(c, 2, "S < 0");
    if (!cov && !c->mvn.valid) return bad_arg(c, 3, "cov is NULL and no factor is cached");
    if (S > 0 && !in) return bad_arg(c, 5, in_is_null);
    if (S > 0 && !out) return bad_arg(c, 6, out_is_null);
    const bool small = fast_path_ok(c, 0, std::max<int64_t>(S, 1));
    return guarded(c, [&]() {
        if (cov) mvn_cache(c, cov, small);   // factor once, keep it in the context
        else if (!small) mvn_tiles_current(c);
        c->last_info.assign((size_t)S, c->mvn.info);
        return body(small);
    });
}

// the S dense-covariance nodes of the single-workgroup path: covscale_s times the cached covariance, target column s
std::vector<HostNode> mvn_nodes(const gpslc_ctx* c, int64_t S, const double* covscale, const double* target) {
    std::vector<HostNode> hn;
    hn.reserve((size_t)S);
    for (int64_t s = 0; s < S; ++s) hn.push_back(dense_node(c->mvn.dense, covscale ? covscale[s] : 1.0, target + s * c->n));
    return hn;
}

}  // namespace

extern "C" {

int gpslc_y_logpdf(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                   const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale,
                   const double* yNoise, double* logpdf) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!logpdf) return bad_arg(c, 11, "logpdf is NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    if (!fast_path_ok(c, c->nU + c->nX + 1, S)) {
        PredictIO io;
        return outcome_call(c, rq, X_or_null, Y_or_null, logpdf, io, {});
    }
    return guarded(c, [&]() {
        // small n: every parameter set is one workgroup of ONE launch (k_small.hip); T enters as a feature column
        const size_t n = (size_t)c->n;
        std::vector<HostNode> hn;
        hn.reserve((size_t)S);
        for (int64_t s = 0; s < S; ++s)
            hn.push_back(y_node(c->nU, U + s * n * c->nU, uyLS + s * c->nU, c->nX, X_or_null ? X_or_null : c->hX.data(),
                                xyLS + s * c->nX, c->hT.data(), tyLS[s], yScale[s], yNoise[s],
                                Y_or_null ? Y_or_null : c->hY.data()));
        return small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
    });
}

// leave-one-out checks from the tile factor gpslc_y_logpdf's general path computes: the tiled path at every n
int gpslc_y_loo(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                double* looMean, double* looVar, double* looLpd, double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!looMean && !looVar && !looLpd && !logpdf_or_null) return bad_arg(c, 11, "looMean, looVar, looLpd and logpdf are all NULL");
    const size_t nS = (size_t)c->n * (size_t)S;
    PredictIO io;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{looMean, &io.loo.mean, nS}, {looVar, &io.loo.var, nS}, {looLpd, &io.loo.lpd, nS}});
}

// gradient of the outcome log-likelihood: gpslc_y_loo's call with other outputs
int gpslc_y_logpdf_grad(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                        const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                        double* dU, double* duyLS, double* dxyLS, double* dtyLS, double* dyScale, double* dyNoise, double* dY,
                        double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!dU && !duyLS && !dxyLS && !dtyLS && !dyScale && !dyNoise && !dY)
        return bad_arg(c, 11, "dU, duyLS, dxyLS, dtyLS, dyScale, dyNoise and dY are all NULL");
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) {
        set_err(c, "gpslc_y_logpdf_grad needs an fp64 context: the pair pass evaluates K in fp64, not the matrix an fp32 context factorises");
        return GPSLC_ERR_UNSUPPORTED;
    }
    if (c->nU == 0) dU = duyLS = nullptr;       // the outputs of an empty block are ignored
    if (c->nX == 0) dxyLS = nullptr;
    const size_t sS = (size_t)S, nS = (size_t)c->n * sS;
    PredictIO io;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{dU, &io.grad.U, nS * (size_t)c->nU}, {duyLS, &io.grad.uyLS, (size_t)c->nU * sS},
                         {dxyLS, &io.grad.xyLS, (size_t)c->nX * sS}, {dtyLS, &io.grad.tyLS, sS}, {dyScale, &io.grad.yScale, sS},
                         {dyNoise, &io.grad.yNoise, sS}, {dY, &io.grad.Y, nS}});
}

// What gpslc_y_lgo and gpslc_y_kfold share: gpslc_y_loo's call with a labelling, every check before any device
// work.  kfold: groups of any size — those beyond LGO_MAX_GROUP take the tiled path (predict.hip, kfold_large); else they are
// refused.
static int group_call(gpslc_ctx* c, bool kfold, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                      const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                      int32_t G, const int32_t* labels, double* gMean, double* gVar, double* gLpd, double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    const int64_t n = c->n;
    if (G < 1 || G > n) return bad_arg(c, 11, "G < 1 or G > n");
    if (!labels) return bad_arg(c, 12, "labels is NULL");
    // the member list sorted by (group, row): a counting sort, rows ascending inside every group
    std::vector<int> offsets((size_t)G + 1, 0), members((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] < 0 || labels[i] >= G) return bad_arg(c, 12, "a label is outside [0, G)");
        ++offsets[(size_t)labels[i] + 1];
    }
    for (int32_t g = 0; g < G; ++g) {
        if (offsets[(size_t)g + 1] == 0) return bad_arg(c, 12, "a group has no member");
        offsets[(size_t)g + 1] += offsets[g];
    }
    if (!gMean && !gVar && !gLpd)
        return bad_arg(c, 13, kfold ? "cvMean, cvVar and cvLpd are all NULL" : "lgoMean, lgoVar and lgoLpd are all NULL");
    PredictIO io;
    io.lgo.G = G;
    io.lgo.kfold = kfold;
    std::vector<int> split;                     // gpslc_y_kfold: the small groups, then the large ones by ascending tile count
    std::vector<std::pair<int, int>> large;     // (tile rows of C, group): sorted, a class is a run of equal tile counts
    for (int32_t g = 0; g < G; ++g) {
        const int m = offsets[(size_t)g + 1] - offsets[g];
        if (m > io.lgo.big_m) { io.lgo.big_m = m; io.lgo.big_group = g; }
        if (m <= LGO_MAX_GROUP) {
            io.lgo.mmax = std::max(io.lgo.mmax, m);
            split.push_back(g);
        } else if (kfold) {
            large.emplace_back((m + GP_TS - 1) / GP_TS, g);
        } else {
            char buf[200];
            snprintf(buf, sizeof buf, "group %d has %d members: gpslc_y_lgo takes groups of at most %d (use gpslc_y_kfold)", (int)g, m,
                     LGO_MAX_GROUP);
            set_err(c, buf);
            return GPSLC_ERR_UNSUPPORTED;
        }
    }
    if (kfold) {
        io.lgo.nsmall = (int)split.size(); io.lgo.nlarge = (int)large.size();
        std::sort(large.begin(), large.end());
        for (const auto& lg : large) {
            if (io.lgo.classes.empty() || io.lgo.classes.back().mt != lg.first) io.lgo.classes.push_back({lg.first, (int)split.size(), 0});
            ++io.lgo.classes.back().count;
            split.push_back(lg.second);
        }
    }
    {
        std::vector<int> fill(offsets.begin(), offsets.end() - 1);
        for (int64_t i = 0; i < n; ++i) members[(size_t)fill[labels[i]]++] = (int)i;
    }
    const size_t nS = (size_t)n * (size_t)S, GS = (size_t)G * (size_t)S;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{gMean, &io.lgo.mean, nS}, {gVar, &io.lgo.var, nS}, {gLpd, &io.lgo.lpd, GS}}, [&]() {
                            auto upload = [&](const std::vector<int>& v) {      // the member list and its offsets
                                int* d = c->io.take<int>(v.size());
                                HC(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
                                return d;
                            };
                            io.lgo.members = upload(members); io.lgo.offsets = upload(offsets);
                            if (kfold) io.lgo.split = upload(split);
                        });
}

// leave-group-out checks, groups of at most LGO_MAX_GROUP members
int gpslc_y_lgo(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                int32_t G, const int32_t* labels, double* lgoMean, double* lgoVar, double* lgoLpd, double* logpdf_or_null) {
    return group_call(c, false, S, U, X_or_null, Y_or_null, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, lgoMean, lgoVar, lgoLpd,
                      logpdf_or_null);
}

// K-fold cross-validation: gpslc_y_lgo for groups of any size
int gpslc_y_kfold(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                  const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                  int32_t G, const int32_t* labels, double* cvMean, double* cvVar, double* cvLpd, double* logpdf_or_null) {
    return group_call(c, true, S, U, X_or_null, Y_or_null, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, cvMean, cvVar, cvLpd,
                      logpdf_or_null);
}

int gpslc_gp_logpdf(gpslc_ctx* c, int64_t S, int32_t nF, const double* F, int32_t f_shared, const double* ls,
                    const double* scale, const double* noise, const double* target, int32_t t_shared,
                    double* logpdf) {
    if (!c) return -1;
    if (S < 0) return bad_arg(c, 2, "S < 0");
    if (nF < 0 || nF > 32) return bad_arg(c, 3, "nF must be in 0..32");
    if (nF > 0 && (!F || !ls)) return bad_arg(c, 4, "F / ls must not be NULL when nF > 0");
    if (S > 0 && (!scale || !noise)) return bad_arg(c, 7, "scale / noise must not be NULL");
    if (S > 0 && !target) return bad_arg(c, 9, "target is NULL");
    if (!logpdf) return bad_arg(c, 11, "logpdf is NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t n = (size_t)c->n;
        if (!fast_path_ok(c, nF, S)) return gp_logpdf_general(c, S, nF, F, f_shared, ls, scale, noise, target, t_shared, logpdf);
        std::vector<HostNode> hn;
        hn.reserve((size_t)S);
        for (int64_t s = 0; s < S; ++s)
            hn.push_back(rbf_node(nF, F + (f_shared ? 0 : s * n * nF), ls + s * nF, scale[s], noise[s], target + (t_shared ? 0 : s * n)));
        return small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
    });
}

int gpslc_nodes_logpdf(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* logpdf) {
    const int nF_max = nodes_check(c, count, nodes, logpdf, "logpdf is NULL");
    return nF_max < 0 ? nF_max : nodes_score(c, count, nodes, nF_max, logpdf, nullptr);
}

// The fused whole-model gradient: the score's single launch with the gradient phases behind it while every node
// fits small_grad_lds_bytes, else — one node that does not fit, more than 4096 nodes — the tiled path for the whole call
int gpslc_nodes_logpdf_grad(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* dF, double* dls, double* dscale,
                            double* dnoise, double* dtarget, double* logpdf_or_null) {
    const NodeGradOut g{dF, dls, dscale, dnoise, dtarget};
    const double* some = g.any() ? (dF ? dF : dls ? dls : dscale ? dscale : dnoise ? dnoise : dtarget) : nullptr;
    const int nF_max = nodes_check(c, count, nodes, some, "dF, dls, dscale, dnoise and dtarget are all NULL");
    if (nF_max < 0) return nF_max;
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) {
        set_err(c, "gpslc_nodes_logpdf_grad needs an fp64 context: the gradient evaluates K in fp64, not the matrix an fp32 context factorises");
        return GPSLC_ERR_UNSUPPORTED;
    }
    if (count == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        std::vector<double> lp;
        double* logpdf = logpdf_or_null;
        if (!logpdf) { lp.resize((size_t)count); logpdf = lp.data(); }
        if (small_grad_lds_bytes((int)c->n, nF_max) > kLdsCapBytes || count > 4096)
            return nodes_general(c, count, nodes, nF_max, logpdf, nullptr, &g);
        std::vector<HostNode> hn;
        hn.reserve((size_t)count);
        for (int i = 0; i < count; ++i) {
            const gpslc_node& q = nodes[i];
            hn.push_back(rbf_node(q.nF, q.F, q.ls, q.scale, q.noise, q.target));
        }
        return small_nodes_logpdf(c, count, hn.data(), logpdf, nullptr, &g);
    });
}

int gpslc_nodes_draw(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* draws, double* logpdf_or_null) {
    const int nF_max = nodes_check(c, count, nodes, draws, "draws is NULL");
    return nF_max < 0 ? nF_max : nodes_score(c, count, nodes, nF_max, logpdf_or_null, draws);
}

int gpslc_mvn_logpdf(gpslc_ctx* c, int64_t S, const double* cov, const double* covscale, const double* x,
                     double* logpdf) {
    return mvn_call(c, S, cov, x, "x is NULL", logpdf, "logpdf is NULL", [&](bool small) {
        if (S == 0 || c->mvn.info != 0) {
            for (int64_t s = 0; s < S; ++s) logpdf[s] = NAN;
            return c->mvn.info;
        }
        if (small) {
            // small n: the dense matrix stays on the device; every evaluation is one workgroup that scales, factorises
            // and solves in LDS (k_small.hip) — cheaper than the tiled forward solve against a cached factor
            const std::vector<HostNode> hn = mvn_nodes(c, S, covscale, x);
            const int st = small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
            if (st > 0) for (int64_t s = 0; s < S; ++s) if (c->last_info[s] != 0) logpdf[s] = NAN;
            return st;
        }
        const int n = (int)c->n;
        const double* oq = mvn_solve_tiles(c, S, x);
        if (c->flags & GPSLC_FLAG_PROFILE) prof_collect(c);
        std::vector<double> q(S);
        HC(hipMemcpy(q.data(), oq, sizeof(double) * S, hipMemcpyDeviceToHost));
        for (int64_t s = 0; s < S; ++s) {
            const double sc = covscale ? covscale[s] : 1.0;
            logpdf[s] = -0.5 * ((double)n * kLog2Pi + (double)n * std::log(sc) + c->mvn.logdet + q[s] / sc);
        }
        return GPSLC_OK;
    });
}

// draws[:, s] = chol(covscale_s cov) z[:, s]: Gen's mvnormal(zeros(n), uCov) with the host's normals — the auxiliary vector of
// elliptical_slice(trace, :U => k => :U, zeros(n), uCov) (src/inference.jl:48-54) and the prior draw generateUfromSigmaU
// (src/model_likelihood.jl:4-10) — from the covariance gpslc_mvn_logpdf caches (chol(s C) = sqrt(s) chol(C))
int gpslc_mvn_draw(gpslc_ctx* c, int64_t S, const double* cov, const double* covscale, const double* z, double* draws) {
    return mvn_call(c, S, cov, z, "z is NULL", draws, "draws is NULL", [&](bool small) {
        const size_t n = (size_t)c->n;
        if (S == 0) return GPSLC_OK;        // a hand-over alone answers GPSLC_OK here; the covariance's info is in last_info
        if (c->mvn.info != 0) {
            for (size_t e = 0; e < n * (size_t)S; ++e) draws[e] = NAN;
            return c->mvn.info;
        }
        if (small) {
            const std::vector<HostNode> hn = mvn_nodes(c, S, covscale, z);
            std::vector<double> lp((size_t)S);
            return small_nodes_logpdf(c, (int)S, hn.data(), lp.data(), draws);
        }
        // tiled: L z on the predictive-draw kernel (every unit streams the ONE cached factor: batch stride 0), scaled on the host
        ensure_streams(c);
        hipStream_t st = c->slots[0].st;
        const int nt = c->nt;
        const long long Np = (long long)nt * GP_TS;
        c->io.reset();
        const double* dz = up(c, z, n * (size_t)S);
        double* zero_mean = c->io.take<double>(n * (size_t)S);
        double* out = c->io.take<double>(n * (size_t)S);
        double* zt = c->io.take<double>((size_t)S * draws_image_doubles(1, Np));
        HC(hipMemsetAsync(zero_mean, 0, n * (size_t)S * sizeof(double), st));
        launch_draws(zero_mean_draw(lower_ref(c->mvn.tiles, 0), (int)n, nt, 0, S, zero_mean, dz, zt, out), (int)S, st);
        HC(hipStreamSynchronize(st));
        HC(hipGetLastError());
        HC(hipMemcpy(draws, out, n * (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
        if (covscale)
            for (int64_t s = 0; s < S; ++s) {
                const double r = std::sqrt(covscale[s]);
                for (size_t i = 0; i < n; ++i) draws[s * n + i] *= r;
            }
        return GPSLC_OK;
    });
}

}  // extern "C"
