// run_predict: the chunk loop of a prediction call and its per-chunk units.
#include "predict.h"
#include "batch_plan.h"

#include <algorithm>
#include <cstdio>
#include <string>

namespace gpslc_host {
namespace {

// chunk and unit-B sub-batch sizes of a call (batch_plan.h holds the arithmetic; here: what the schedule would like and what
// the device has)
BatchPlan auto_batch(gpslc_ctx* c, int64_t S, int L, size_t per_sample_bytes, size_t unit_bytes, size_t lvl_extra) {
    // enough matrices in flight that the per-step diagonal-block kernel (one workgroup per matrix) and the
    // launch quantisation of the late, small trailing updates are amortised: 1024 at N = 4096 (82 GB of the
    // 288 GB; measured 2013 / 2040 / 2055 / 2064 samples/s at batch 256 / 512 / 1024 / 2048)
    // small matrices: up to 16,384 per chunk (N = 1024: 4,096 / 8,192 / 16,384 per chunk -> 83.8 k / 84.6 k / 86.5 k samples/s,
    // profiles/r04_ab_experiments.md §16 — every launch's ramp and tail are amortised over more items); memory permitting
    long long b = 1048576LL / ((long long)c->nt * c->nt);
    b = std::max<long long>(32, std::min<long long>(b, 16384));
    if (c->max_batch > 0) b = c->max_batch;
    // unit-B sub-batch (unit_bytes > 0): 128 units at N = 4096 (203 MB each, 26 GB).  Round 5, 256 units of 8 samples x 32 levels
    // on one box (profiles/r05_ab_experiments.md §3): 16 / 32 / 64 / 128 / 256 per sub-batch -> 322 / 349 / 364 / 372 / 373
    // units/s — the late columns of a factorisation have (nt - k) x sub-batch items for 512 workgroup slots; flat from 128 on
    const long long want_bb = std::max<long long>(1, std::min<long long>(128, 131072LL / ((long long)c->nt * c->nt)));
    size_t free_b = 0, tot_b = 0;
    HC(hipMemGetInfo(&free_b, &tot_b));
    size_t have = 0;
    for (auto& sl : c->slots) have += sl.arena.bytes();
    // the AUTOMATIC chunk also stays under 30 % of the device's memory (arenas never shrink, and the host process usually
    // shares the device: torch's caching allocator under sharded.py / bench.py, other contexts of gpslc_predict_multi on one
    // GPU); 1,024 matrices at N = 4096 are 28 %.  gpslc_set_tuning(max_batch) may ask for more: then only what is free counts.
    const BatchPlan p = plan_batch(b, want_bb, S, L, per_sample_bytes, unit_bytes, lvl_extra, free_b, have, tot_b, c->nstreams,
                                   c->max_batch <= 0);
    if (!p.ok) throw std::bad_alloc();
    return p;
}

// what one run_predict call computes and the sizes that follow from it (the same for all of its chunks)
struct PredictShape {
    int n, nt, L, R, naug, ntot;      // R: right-hand sides beside Y — one per level, or L*G with weight columns
    long long Np, tiles_per, nlow;   // padded N, tiles of A with its augmented rows, tiles of an nt x nt triangle
    bool with_sums, want_cov, want_draws, want_mean, unitB;     // unitB: full ITE covariance (CovITE, draws)
    bool want_loo, want_lgo;          // leave-one-out outputs, leave-group-out outputs
    bool want_grad, grad_pairs, grad_c;   // gradient outputs; those that need the pass over the pairs (U and the lengthscales'); those
                                      // that need c = diag(A^-1) (yScale, yNoise)
    bool want_w;                      // W = L^-T is wanted (by any of them)
    bool want_alpha;                  // alpha = A^-1 Y is wanted (by the MeanITE pass or by them)
    bool mean_operands;               // the MeanITE pass runs from the chunk's operand array (ite_mean_uses_operands)
    bool gram_operands;               // ... and so does the Gram build (gram_uses_operands): unit_a fills the array, else mean_ite
    int mt;                           // new individuals: their row tiles, the tiles of an mt x mt triangle, and whether the
    long long mlow;                   // (sample, level) pairs need tile workspace (variance, covariance)
    bool want_new, new_pairs;
    bool kfold_pairs;                 // gpslc_y_kfold with groups beyond LGO_MAX_GROUP: (group, sample) pairs with tile workspace
    int kf_mt;                        // ... and the tile rows of the largest group's C
    PredictShape(const gpslc_ctx* c, const PredictIO& io)
        : n((int)c->n), nt(c->nt), L(io.lv.L), R(io.lv.W ? io.lv.L * io.lv.G : io.lv.L), naug((R + 1 + GP_TS - 1) / GP_TS), ntot(nt + naug),
          Np((long long)nt * GP_TS), tiles_per((long long)ntot * (ntot + 1) / 2), nlow((long long)nt * (nt + 1) / 2),
          with_sums(io.out.meanSATE || io.out.varSATE || io.out.covW), want_cov(io.CovITEs != nullptr), want_draws(io.out.ite_draws != nullptr),
          want_mean(io.out.meanITE || io.MeanITEs || want_draws), unitB(want_cov || want_draws),
          want_loo(io.loo.any()), want_lgo(io.lgo.any()), want_grad(io.grad.any()), grad_pairs(io.grad.pairs()),
          grad_c(io.grad.needs_c()), want_w(want_loo || want_lgo || want_grad), want_alpha(want_mean || want_w || io.fresh.mean),
          mean_operands(want_mean && !io.lv.vec && ite_mean_uses_operands(io.nU + io.nX, io.lv.L, (c->flags & GPSLC_FLAG_FP32_KERNEL) != 0)),
          gram_operands(gram_uses_operands(io.nU + io.nX, (c->flags & GPSLC_FLAG_FP32_KERNEL) != 0)),
          mt((io.fresh.m + GP_TS - 1) / GP_TS), mlow((long long)mt * (mt + 1) / 2), want_new(io.fresh.any()),
          new_pairs(io.fresh.pairs()), kfold_pairs(io.lgo.any() && io.lgo.kfold && io.lgo.nlarge > 0), kf_mt(io.lgo.mt_max()) {}
};

// one chunk of a call: samples s0 .. s0 + nb - 1 on one stream slot, and the buffers carve_chunk takes for it from the slot's arena
struct Chunk {
    StreamSlot* s = nullptr;
    int64_t s0 = 0;
    int nb = 0;
    TRef M{};                        // the tile matrices of A over `tiles`
    double *tiles = nullptr, *inv = nullptr, *part = nullptr, *bsum = nullptr, *ksum = nullptr, *sumdelta = nullptr;
    double *vpart = nullptr, *zwork = nullptr, *znode = nullptr;
    double *cop = nullptr, *rlev = nullptr;      // MeanITE from scalar operands: ColOperandArgs::cop [nb][Np][FP], IteMeanArgs::R [nb][Np][LCT]
    double *bw = nullptr, *kw = nullptr, *wnorm2 = nullptr;      // weighted effects: B W, K W [nb][G][Np], w_g . w_g [nb][G]
    double* cprior = nullptr;        // joint covariance across the levels: beta, kappa, gamma_l [nb][G][L + 2]
    double* wpart = nullptr;         // weighted averages over new individuals: the row blocks' shares of w' B** w [nb][mt][G]
    double *loo_w = nullptr, *loo_c = nullptr;      // leave-one-out: W = L^-T as a packed triangle of tiles [nb][nlow], diag(A^-1) [nb][Np]
    double *grad_ls = nullptr, *grad_u = nullptr;   // gradient: the pair pass's partial sums per tile (GradArgs::part_ls, part_u)
    // unit B: a sub-batch of gs_max samples x lc_max levels; W, CovITE, the draws' normals, level-sweep staging, failure codes
    int lc_max = 0, gs_max = 0;
    double *Wt = nullptr, *Ct = nullptr, *zt = nullptr, *dtmp = nullptr;
    int* pinfo = nullptr;
    // gpslc_y_kfold's large groups: a sub-batch of kf_max (group, sample) pairs; C with its augmented row, its inverted diagonal
    // tiles, its L^-T, [z | C^-1 alpha_I] (launch_backsolve's layout), diag(C^-1), log det C and the quadratic form, failure codes
    int kf_max = 0;
    double *kf_c = nullptr, *kf_inv = nullptr, *kf_w = nullptr, *kf_zu = nullptr, *kf_diag = nullptr, *kf_ldq = nullptr;
    SampleGrid grid{};               // the chunk's samples and feature blocks, as every RBF-evaluating kernel takes them
};

struct ChunkBytes { size_t per_sample = 1024, per_pair = 0, per_level = 0; };    // 1 KiB: the 256-byte alignment of each buffer

// Carves a chunk's buffers from its slot's arena (nb samples, sub-batches of Bb pairs) and counts, beside each buffer, the bytes
// auto_batch reserves for it: per sample, per (sample, level) pair of a unit-B sub-batch, and per level of a sweep beyond the
// sub-batch (the level-sweep staging).  ch == nullptr: the counts only.
ChunkBytes carve_chunk(const PredictShape& sh, const PredictIO& io, int Bb, Chunk* ch) {
    ChunkBytes by;
    Chunk none;
    Chunk& b = ch ? *ch : none;
    Arena<DeviceMem>* ar = ch ? &ch->s->arena : nullptr;
    auto take = [&](size_t per_sample) -> double* {
        by.per_sample += per_sample * 8;
        return ar ? ar->take<double>((size_t)b.nb * per_sample) : nullptr;
    };
    const int n = sh.n, nt = sh.nt, L = sh.L;
    // the streaming draw kernel reads a pass's normals (caller's or Philox) from the unit's operand image (DrawArgs::zt)
    const size_t zimage_doubles = sh.want_draws ? draws_image_doubles(io.out.spp, sh.Np) : 0;
    b.tiles = take(sh.tiles_per * GP_TSQ);
    b.inv = take((size_t)nt * GP_TSQ);
    if (sh.with_sums && !io.lv.W) b.part = take(2 * nt * sh.Np);
    b.bsum = take(sh.Np); b.ksum = take(sh.Np);
    b.sumdelta = take(std::max(sh.R, 1));
    if (io.lv.W) {      // only the factual form needs K W
        b.bw = take((size_t)io.lv.G * sh.Np);
        b.kw = io.lv.needs_kw() ? take((size_t)io.lv.G * sh.Np) : b.bw;
        b.wnorm2 = take(io.lv.G);
        if (io.out.covW) b.cprior = take((size_t)io.lv.G * (L + 2));
        if (io.fresh.weighted) b.wpart = take((size_t)sh.mt * io.lv.G);
    }
    if (io.lv.vec && sh.with_sums) b.vpart = take((size_t)L * nt);     // vector levels: per-tile shares of sum(Delta)
    b.zwork = take(2 * sh.Np);                                          // zwork + alpha
    // the scalar-operand pair kernels: the operand array (Gram build, MeanITE pass) and the level vectors R (MeanITE pass)
    if (sh.gram_operands || sh.mean_operands) b.cop = take((size_t)sh.Np * col_operand_width(io.nU + io.nX));
    if (sh.mean_operands) b.rlev = take((size_t)sh.Np * ite_mean_lct(L));
    if (io.ndraw) b.znode = take(draws_image_doubles(1, sh.Np));        // operand image of the node draw's normals
    if (sh.want_w) b.loo_w = take((size_t)sh.nlow * GP_TSQ);
    if (sh.want_loo || sh.grad_c) b.loo_c = take(sh.Np);
    if (sh.grad_pairs) {      // F numbers per lower tile; 128 nU per (tile row, tile column)
        b.grad_ls = take((size_t)sh.nlow * (io.nU + io.nX + (io.grad_no_t ? 0 : 1)));
        if (io.nU > 0) b.grad_u = take((size_t)nt * nt * io.nU * GP_TS);
    }
    b.M = lower_ref(b.tiles, sh.tiles_per * GP_TSQ);
    if (sh.kfold_pairs) {     // sized for the largest group: a class of fewer tile rows uses the front of every buffer
        const size_t mt = (size_t)sh.kf_mt, c_tiles = (mt + 1) * (mt + 2) / 2, w_tiles = mt * (mt + 1) / 2, Nc = mt * GP_TS;
        by.per_pair = (c_tiles + mt + w_tiles) * GP_TSQ * 8 + (3 * Nc + 2) * 8 + sizeof(int);
        if (!ar) return by;
        b.kf_max = Bb;
        b.kf_c = ar->take<double>((size_t)Bb * c_tiles * GP_TSQ);
        b.kf_inv = ar->take<double>((size_t)Bb * mt * GP_TSQ);
        b.kf_w = ar->take<double>((size_t)Bb * w_tiles * GP_TSQ);
        b.kf_zu = ar->take<double>((size_t)Bb * 2 * Nc);
        b.kf_diag = ar->take<double>((size_t)Bb * Nc);
        b.kf_ldq = ar->take<double>((size_t)Bb * 2);
        b.pinfo = ar->take<int>((size_t)Bb);
        return by;
    }
    if (sh.new_pairs) {       // new individuals: W* (mt x nt) and, with the covariance, an mt triangle per (sample, level) pair
        // the joint density of a test set factorises C in place: one more tile row for its augmented row, the
        // inverted diagonal tiles, log det C and the quadratic form, a failure code
        const bool joint = io.fresh.lpd_joint != nullptr;
        const size_t w_tiles = (size_t)sh.mt * nt, mt = (size_t)sh.mt;
        const size_t c_tiles = joint ? (mt + 1) * (mt + 2) / 2 : io.fresh.cov ? (size_t)sh.mlow : 0;
        by.per_pair = (w_tiles + c_tiles + (joint ? mt : 0)) * GP_TSQ * 8 + 512 + (joint ? 3 * 256 : 0);
        if (!ar) return by;
        b.lc_max = std::min(L, Bb);
        b.gs_max = std::max(1, Bb / b.lc_max);
        b.Wt = ar->take<double>((size_t)Bb * w_tiles * GP_TSQ);
        if (c_tiles) b.Ct = ar->take<double>((size_t)Bb * c_tiles * GP_TSQ);
        if (joint) {
            b.kf_inv = ar->take<double>((size_t)Bb * mt * GP_TSQ);
            b.kf_ldq = ar->take<double>((size_t)Bb * 2);
            b.pinfo = ar->take<int>((size_t)Bb);
        }
        return by;
    }
    if (!sh.unitB) return by;
    by.per_pair = (size_t)((long long)nt * nt + sh.nlow) * GP_TSQ * 8;
    if (sh.want_draws) {
        by.per_pair += zimage_doubles * 8 + 256 + (L > 1 ? (size_t)io.out.spp * n * 8 + 256 : 0) + sizeof(int) + 256;
        by.per_level = (size_t)io.out.spp * n * 8;
    }
    if (!ar) return by;
    b.lc_max = std::min(L, Bb);                      // levels per sub-batch
    b.gs_max = std::max(1, Bb / b.lc_max);           // samples per sub-batch
    b.Wt = ar->take<double>((size_t)Bb * nt * nt * GP_TSQ);
    b.Ct = ar->take<double>((size_t)Bb * sh.nlow * GP_TSQ);
    // draws: the operand images of one sub-batch, and for a level sweep the staging buffer
    // [sample][level][d][i] that is rearranged into the level-fastest tensor sample group by group (per unit of the sub-batch:
    // max(1, Bb / L) samples x L levels <= Bb pairs, or one sample's L > Bb levels — per_level)
    if (sh.want_draws) b.zt = ar->take<double>((size_t)Bb * zimage_doubles);
    if (sh.want_draws && L > 1) b.dtmp = ar->take<double>((size_t)b.gs_max * L * io.out.spp * n);
    // failure codes of the CovITE factors, one per pair of a sub-batch (folded into io.info after each sub-batch)
    if (sh.want_draws) b.pinfo = ar->take<int>((size_t)Bb);
    return by;
}

// the vector-level kernels' arguments of a chunk (doT is n x L: level l at doT + n*l)
VecArgs vec_args(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    VecArgs va{ch.grid};
    va.lv = io.lv.set(sh.L);
    va.M = ch.M; va.part = ch.vpart; va.sumdelta = ch.sumdelta;
    va.Y = io.Y; va.y_sstride = io.y_sstride;
    return va;
}

}  // namespace

// One draw per unit from N(0, L L^T): unit b streams the factor Lc of batch element b (batch stride 0: ONE factor for all) and
// multiplies it with column s0 + b of the normals z (n x S); `zero` is n x S zeros (the draw kernel's mean), zt the operand
// image workspace, out n x S.
DrawArgs zero_mean_draw(TRef Lc, int n, int nt, long long s0, long long S, const double* zero, const double* z, double* zt,
                        double* out) {
    DrawArgs dr{};
    dr.Lc = Lc; dr.n = n; dr.nt = nt; dr.s0 = s0; dr.S = S; dr.l = 0; dr.lc = 1; dr.L = 1; dr.spp = 1;
    dr.mean = zero; dr.z = z; dr.zt = zt; dr.out = out;
    dr.obase = (long long)n * s0; dr.osb = n; dr.osl = 0; dr.osi = 1; dr.osd = n;
    return dr;
}

namespace {

// unit A of a chunk: Gram build, right-hand sides, vector sums, factorisation, epilogue and node draw.  Returns whether the
// factorisation delivered the back-substitution alpha.
bool unit_a(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nt = sh.nt, nb = ch.nb;
    const int64_t s0 = ch.s0;
    GramArgs ga{ch.grid};
    ga.M = ch.M; ga.part = ch.part;
    ga.with_sums = (sh.with_sums && !io.lv.W) ? 1 : 0;      // weighted: the column sums come from launch_wsum instead
#ifdef GPSLC_DIAG
    static const int gram_dbg = diag_env("GPSLC_GRAM_DBG", 0);
    static bool gram_dbg_done = false;
    StampCapture stamps;
    if (gram_dbg && !gram_dbg_done) ga.dbg = stamps.arm((size_t)8 * nb * (nt * (nt + 1) / 2));
#endif
    ga.f32 = (c->flags & GPSLC_FLAG_FP32_KERNEL) ? 1 : 0;
    ga.binary_t = (c->binary_t && io.nU == c->nU && io.nX == c->nX && io.Y == c->dY) ? 1 : 0;   // ctx data only
    if (sh.gram_operands) {      // once per chunk, before the Gram build: the operand array both pair kernels read
        ColOperandArgs ca{ch.grid};
        ca.cop = ch.cop;
        launch_col_operands(ca, nb, st);
        ga.cop = ch.cop;
    }
    const bool over_new = io.fresh.weighted;      // the weight columns run over the new individuals
    if (over_new) {     // B*' W over the m x n pairs, w' B** w over the m x m pairs, and the sums the prepare kernels would form
        NewWsumArgs wa{};
        static_cast<SampleGrid&>(wa) = ch.grid;
        wa.Xnew = io.fresh.Xnew; wa.Unew = io.fresh.Unew; wa.un_sstride = (long long)io.fresh.m * io.nU; wa.m = io.fresh.m; wa.mt = sh.mt;
        wa.lv = io.lv.set(sh.L); wa.G = io.lv.G; wa.W = io.lv.W;
        wa.bw = ch.bw; wa.part = ch.wpart; wa.sumdelta = ch.sumdelta; wa.wnorm2 = ch.wnorm2; wa.prior = ch.cprior;
        launch_new_wsum(wa, nb, st);
    } else if (io.lv.W) {      // weighted effects: B W and K W, one pass over the pairs for all columns and levels (independent of the tiles)
        WsumArgs wa{ch.grid};
        wa.G = io.lv.G; wa.W = io.lv.W;
        wa.bw = ch.bw; wa.kw = ch.kw; wa.with_k = io.lv.needs_kw() ? 1 : 0; wa.binary_t = ga.binary_t;
        launch_wsum(wa, nb, st);
    }
    launch_gram(ga, nb, st);
#ifdef GPSLC_DIAG
    if (ga.dbg) {      // GPSLC_GRAM_DBG: dump the first launch's per-workgroup stamps
        FILE* f = fopen("gpurun_out/gram_dbg.bin", "wb");
        stamps.dump(st, f);
        gram_dbg_done = true;
    }
#endif
    RhsArgs ra{};
    ra.T = c->dT; ra.Y = io.Y; ra.y_sstride = io.y_sstride; ra.tyLS = io.post.p.tyLS; ra.s0 = s0;
    // vector levels: rhs_tiles writes zeros into the level rows and rhs_prepare no level sums (no levels here); launch_vec_sums
    // fills both below
    ra.lv = io.lv.set((sh.with_sums && !io.lv.vec) ? sh.L : 0);
    ra.n = n; ra.nt = nt; ra.naug = sh.naug; ra.with_sums = sh.with_sums ? 1 : 0;
    ra.part = ch.part; ra.bsum = ch.bsum; ra.ksum = ch.ksum; ra.sumdelta = ch.sumdelta; ra.M = ch.M;
    const bool epi_rows = (sh.naug == 1);                    // single augmented tile row: the epilogue sums from the rows of R
    const int live = (sh.with_sums ? sh.R : 0) + 1;          // right-hand sides: Y and one c_l per level (and weight column)
    ra.live_rows = (epi_rows && live <= 32) ? 16 * ((live + 15) / 16) : 0;
    ra.G = 1; ra.bw = ch.bsum; ra.kw = ch.ksum;       // the plain call: one column of level sums, the Gram build's
    if (io.lv.W) { ra.W = over_new ? nullptr : io.lv.W; ra.G = io.lv.G; ra.bw = ch.bw; ra.kw = ch.kw; ra.wnorm2 = ch.wnorm2; }
    launch_rhs(ra, nb, st, over_new);
    if (io.lv.vec && sh.with_sums) launch_vec_sums(vec_args(io, sh, ch), nb, st);
    // NB: the MeanITE pass takes K alpha as Y - yNoise alpha (k_solve.hip, ite_mean_kernel): it relies on alpha solving EXACTLY
    // (K_gram + yNoise I) alpha = Y.  Any future jitter, robust fallback or different right-hand side in this factorisation must
    // be reflected there (tests: test_mean_ite_tiny_noise_and_near_coincident_levels).
    const int short_rows = sh.naug == 1 ? live : 0;
    bool back_done = false;
    if (potrf_tasks_ok(c, nt, sh.ntot, short_rows, epi_rows, nb, ch.inv)) {
        // small tile counts: the whole factorisation (and the back-substitution) as ONE persistent launch of tile tasks
        potrf_tasks(c, *ch.s, ch.M, nt, ch.inv, io.info + s0, 0, nb, short_rows,
                    sh.want_alpha ? ch.zwork + (long long)nb * sh.Np : nullptr);
        back_done = sh.want_alpha;
    } else {
        factor_panels(c, *ch.s, ch.M, nt, sh.ntot, ch.inv, io.info + s0, 0, nb, live, epi_rows, 0);
    }
    EpiArgs ea{};
    ea.M = ch.M; ea.n = n; ea.nt = nt; ea.naug = sh.naug; ea.L = sh.with_sums ? sh.R : 0; ea.s0 = s0; ea.S = io.post.S;
    ea.sumdelta = ch.sumdelta; ea.pred_noise = io.out.pred_noise;
    ea.meanSATE = io.out.meanSATE; ea.varSATE = io.out.varSATE; ea.logdet = io.logdet; ea.quad = io.quad;
    ea.from_rows = epi_rows ? 1 : 0;
    if (io.lv.W) { ea.wnorm2 = ch.wnorm2; ea.wL = sh.L; }
    launch_epilogue(ea, nb, st);
    if (io.out.covW) {      // the levels' joint covariance per weight column: Gram matrix of the rows the factorisation carried
        CurveArgs ca{};
        ca.M = ch.M; ca.n = n; ca.nt = nt; ca.lv = io.lv.set(sh.L); ca.G = io.lv.G; ca.s0 = s0; ca.S = io.post.S;
        ca.T = c->dT; ca.tyLS = io.post.p.tyLS;
        ca.W = io.lv.W; ca.bw = ch.bw; ca.kw = ch.kw; ca.prior = ch.cprior;
        ca.varW = io.out.varSATE; ca.covW = io.out.covW;
        launch_curve(ca, nb, st, over_new);
    }
    if (io.ndraw) {
        // one draw from N(0, A_s) per parameter set with the caller's normals: L_s z_s on the factor just computed — Gen's
        // mvnormal(zeros(n), cov) of an elliptical slice's auxiliary vector (src/inference.jl:225-232) and of the :logitT prior
        // draw (src/model_likelihood.jl:25-33) — the predictive-draw kernel streaming L once
        launch_draws(zero_mean_draw(ch.M, n, nt, s0, io.post.S, io.nzero, io.nz, ch.znode, io.ndraw), nb, st);
    }
    return back_done;
}

// alpha = A^-1 Y of a chunk where the factorisation did not deliver it: the back-substitution
void back_substitute(const PredictShape& sh, const Chunk& ch) {
    BackArgs ba{};
    ba.M = ch.M; ba.inv = ch.inv; ba.inv_bstride = (long long)sh.nt * GP_TSQ; ba.nt = sh.nt; ba.naug = sh.naug; ba.zwork = ch.zwork;
    launch_backsolve(ba, ch.nb, ch.s->st);
}

// MeanITE of a chunk from alpha: the ITE-mean kernels, once per output layout asked for: meanITE n x S x L, MeanITEs S x n (the
// reference layout, single level)
void mean_ite(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nb = ch.nb;
    const double* alpha = ch.zwork + (long long)nb * sh.Np;
    const long long S = io.post.S;
    const struct { double* out; long long si, ss, sl; } outs[2] = {{io.out.meanITE, 1, n, (long long)n * S}, {io.MeanITEs, S, 1, 0}};
    if (io.lv.vec) {
        VecArgs va = vec_args(io, sh, ch);
        va.alpha = alpha;
        for (const auto& o : outs)
            if (o.out) { va.meanITE = o.out; va.si = o.si; va.ss = o.ss; va.sl = o.sl; launch_vec_mean(va, nb, st); }
        return;
    }
    IteMeanArgs ia{ch.grid};
    ia.S = S; ia.lv = io.lv.set(sh.L); ia.alpha = alpha;
    ia.Y = io.Y; ia.y_sstride = io.y_sstride; ia.yNoise = io.post.p.yNoise;
    ia.f32 = (c->flags & GPSLC_FLAG_FP32_KERNEL) ? 1 : 0;
    if (sh.mean_operands) {      // once per chunk: the columns' features (unless the Gram build left them), and cross(l) alpha of every column
        if (!sh.gram_operands) {
            ColOperandArgs ca{ch.grid};
            ca.cop = ch.cop;
            launch_col_operands(ca, nb, st);
        }
        ia.cop = ch.cop; ia.R = ch.rlev;
        launch_ite_levels(ia, nb, st);
    }
    for (const auto& o : outs)
        if (o.out) { ia.meanITE = o.out; ia.si = o.si; ia.ss = o.ss; ia.sl = o.sl; launch_ite_mean(ia, nb, st); }
}

}  // namespace

// unit B's W <- D L^-T for ub (sample, level) pairs, left-looking over the whole width: one strip launch per tile column (column
// update + panel product with inv(L_kk)^T in the same work item; column 0 takes the panel product alone), which measured level
// with blocking it like the factorisation (profiles/r04_ab_experiments.md §7).  W has `rows` tile rows: nt for unit B's D, the
// row tiles of the new individuals for D* (unit_new).
void w_solve(gpslc_ctx* c, StreamSlot& s, const TRef& W, const TRef& Ls, const TRef& invref, int nt, int ub, int rows) {
    for (int k = 0; k < nt; ++k) gemm(c, fused(tile_column(W, Ls, W, 0, k, rows, 0, k, ub, false), invref, k), s, 3);
}

namespace {

// what LooArgs, LgoArgs and GradArgs share: the chunk's W = L^-T, alpha = A^-1 Y, the scored Y and the samples' failure codes
template <class Args>
Args on_w(const PredictIO& io, const PredictShape& sh, const Chunk& ch, Args a = Args{}) {
    a.W = ch.loo_w; a.w_bstride = sh.nlow * GP_TSQ; a.n = sh.n; a.nt = sh.nt; a.s0 = ch.s0;
    a.alpha = ch.zwork + (long long)ch.nb * sh.Np; a.Y = io.Y; a.y_sstride = io.y_sstride; a.info = io.info;
    return a;
}

// Leave-one-out predictive checks of a chunk: c = diag(A^-1) as the squared row norms of W = L^-T, then the
// outputs from alpha, c and Y; and / or its leave-group-out checks (§20) from the same W and alpha.  The gradient (§21, grad() below) reads W,
// alpha and c as this function leaves them.  W is built block diagonal by block diagonal, one launch each: diagonal d holds the tiles
// (i, i + d) of all tile rows and matrices, each a chain of d tile products from kk = i on (nt^3/6 products in all, the
// factorisation's count); the tile rows of a matrix are independent chains, so nt x nb of them are in flight.
void loo(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int nt = sh.nt, nb = ch.nb;
    LooArgs la = on_w<LooArgs>(io, sh, ch);
    la.inv = ch.inv; la.inv_bstride = (long long)nt * GP_TSQ;
    la.S = io.post.S; la.c = ch.loo_c;
    la.looMean = io.loo.mean; la.looVar = io.loo.var; la.looLpd = io.loo.lpd;
    HC(hipMemsetAsync(ch.loo_w, 0, sizeof(double) * (size_t)nb * sh.nlow * GP_TSQ, st));     // every chain starts from a zero tile
    launch_loo_init(la, nb, st);
    rearm_queue(*ch.s);
    const TRef W = lower_ref(ch.loo_w, la.w_bstride), invref = inv_ref(ch.inv, nt);
    // a fused column of nt - d items; the kernel gives item i its own tile (i, i + d), K range and inverted block
    for (int d = 1; d < nt; ++d)
        launch_loo_diagonal(on_slot(fused(tile_column(W, ch.M, W, 0, 0, nt - d, 0, 0, nb, false), invref, 0), *ch.s), nt, d, st);
    if (sh.want_loo || sh.grad_c) launch_loo_rownorm(la, nb, st);
    if (sh.want_loo) launch_loo_finish(la, nb, st);
    if (sh.want_lgo) {      // leave-group-out: one workgroup per (group, sample) on the same W and alpha
        LgoArgs ga = on_w<LgoArgs>(io, sh, ch);
        ga.G = io.lgo.G; ga.mmax = io.lgo.mmax; ga.members = io.lgo.members; ga.offsets = io.lgo.offsets;
        ga.lgoMean = io.lgo.mean; ga.lgoVar = io.lgo.var; ga.lgoLpd = io.lgo.lpd;
        if (io.lgo.kfold) { ga.gmap = io.lgo.split; ga.ngroups = io.lgo.nsmall; }      // the larger groups: kfold_large below
        launch_lgo_groups(ga, nb, st);
    }
    HC(hipGetLastError());
}

// gpslc_y_kfold's groups of more than LGO_MAX_GROUP members, after loo() has left W and alpha of the chunk.  Per
// class of equal tile count mt, sub-batches of (group, sample) pairs: C = W[I, :] W[I, :]^T into the pair's tiles with alpha_I as
// the augmented row (launch_kfold_gram); the panel schedule's factorisation of C with the forward solve it carries; log det C and
// the quadratic form from the epilogue, C^-1 alpha_I from the back-substitution, diag(C^-1) as the squared row norms of C's own
// L^-T (loo()'s launches on C's factor); kfold_finish_kernel writes the outputs.  Everything of a pair depends on its member set
// and its sample alone: the sub-batch, the class and the chunk only decide which launch carries it.
void kfold_large(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    KfoldArgs ka = on_w<KfoldArgs>(io, sh, ch);
    ka.G = io.lgo.G; ka.members = io.lgo.members; ka.offsets = io.lgo.offsets;
    ka.cvMean = io.lgo.mean; ka.cvVar = io.lgo.var; ka.cvLpd = io.lgo.lpd;
    for (const Lgo::Class& cl : io.lgo.classes) {
        const int mt = cl.mt;
        const long long c_bs = (long long)(mt + 1) * (mt + 2) / 2 * GP_TSQ, w_bs = (long long)mt * (mt + 1) / 2 * GP_TSQ,
                        inv_bs = (long long)mt * GP_TSQ, Nc = (long long)mt * GP_TS, pairs = (long long)cl.count * ch.nb;
        ka.large = io.lgo.split + cl.first; ka.ng = cl.count; ka.mt = mt;
        ka.Cm = lower_ref(ch.kf_c, c_bs);
        for (long long p0 = 0; p0 < pairs; p0 += ch.kf_max) {
            const int ub = (int)std::min<long long>(ch.kf_max, pairs - p0);
            ka.p0 = p0;
            launch_kfold_gram(ka, ub, st);
            HC(hipMemsetAsync(ch.pinfo, 0, sizeof(int) * ub, st));
            factor_panels(c, *ch.s, ka.Cm, mt, mt + 1, ch.kf_inv, ch.pinfo, 0, ub, 1, true, 3);
            EpiArgs ea{};
            ea.M = ka.Cm; ea.n = (int)Nc; ea.nt = mt; ea.naug = 1; ea.from_rows = 1;
            ea.logdet = ch.kf_ldq; ea.quad = ch.kf_ldq + ub;       // sample index = batch element: s0 = 0
            launch_epilogue(ea, ub, st);
            BackArgs ba{};
            ba.M = ka.Cm; ba.inv = ch.kf_inv; ba.inv_bstride = inv_bs; ba.nt = mt; ba.naug = 1; ba.zwork = ch.kf_zu;
            launch_backsolve(ba, ub, st);
            LooArgs la{};
            la.inv = ch.kf_inv; la.inv_bstride = inv_bs; la.W = ch.kf_w; la.w_bstride = w_bs; la.nt = mt; la.c = ch.kf_diag;
            HC(hipMemsetAsync(ch.kf_w, 0, sizeof(double) * (size_t)ub * w_bs, st));
            launch_loo_init(la, ub, st);
            rearm_queue(*ch.s);
            const TRef W = lower_ref(ch.kf_w, w_bs), invref = inv_ref(ch.kf_inv, mt);
            for (int d = 1; d < mt; ++d)
                launch_loo_diagonal(on_slot(fused(tile_column(W, ka.Cm, W, 0, 0, mt - d, 0, 0, ub, false), invref, 0), *ch.s), mt, d, st);
            launch_loo_rownorm(la, ub, st);
            ka.u = ch.kf_zu + (long long)ub * Nc; ka.cdiag = ch.kf_diag; ka.logdet = ea.logdet; ka.quad = ea.quad; ka.pinfo = ch.pinfo;
            launch_kfold_finish(ka, ub, st);
        }
    }
    HC(hipGetLastError());
}

// Gradient of the outcome log-likelihood of a chunk, after loo() has left W, alpha and, where asked, c: the pass
// over the lower tiles of A^-1 = W W^T (nt^3/6 tile products, the factorisation's count) when U's or a lengthscale's gradient is
// asked, then the kernel that adds the tiles' partial sums and writes every output.  gyScale, gyNoise and gY alone need no pair pass.
void grad(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    GradArgs ga = on_w(io, sh, ch, GradArgs{ch.grid});
    ga.S = io.post.S; ga.c = ch.loo_c;
    ga.part_ls = ch.grad_ls; ga.part_u = ch.grad_u; ga.queue = ch.s->queue;
    ga.dU = io.grad.U; ga.duyLS = io.grad.uyLS; ga.dxyLS = io.grad.xyLS; ga.dtyLS = io.grad.tyLS;
    ga.dyScale = io.grad.yScale; ga.dyNoise = io.grad.yNoise; ga.dY = io.grad.Y;
    ga.no_t = io.grad_no_t ? 1 : 0;
    if (sh.grad_pairs) {
        rearm_queue(*ch.s);
        launch_grad_pairs(ga, ch.nb, st);
    }
    launch_grad_finish(ga, ch.nb, st);
    HC(hipGetLastError());
}

// The pair workspaces of a chunk (unit B's CovITE, the new individuals' variance and covariance) batch over (posterior sample,
// level) PAIRS: a sub-batch is gs samples x lc levels (gs * lc = ub <= Bb), batch element b = (sample g0 + b / lc, level l0 +
// b % lc).  Every pair has its own tiles; the factor of A (Ls) and its inverted diagonal blocks (invref) are shared by a
// sample's levels (TRef::bdiv = lc) — the shape of predictCounterfactualEffects (src/prediction.jl:30-33): few samples, ~100 levels.
template <class Body>
void for_pair_batches(const PredictShape& sh, const Chunk& ch, Body&& body) {
    const long long bstride = sh.tiles_per * GP_TSQ, inv_bs = (long long)sh.nt * GP_TSQ;
    for (int g0 = 0; g0 < ch.nb; g0 += ch.gs_max) {
        const int gs = std::min(ch.gs_max, ch.nb - g0);
        for (int l0 = 0; l0 < sh.L; l0 += ch.lc_max) {
            const int lc = std::min(ch.lc_max, sh.L - l0);
            TRef Ls = lower_ref(ch.tiles + (long long)g0 * bstride, bstride);
            TRef invref = inv_ref(ch.inv + (long long)g0 * inv_bs, sh.nt);
            Ls.bdiv = invref.bdiv = lc;
            body(g0, gs, l0, lc, gs * lc, Ls, invref);
        }
    }
}

// C <- C - W W^T on the lower tiles of C's `rows` tile rows, for ub pairs (W: rows x nt tiles)
void minus_w_wt(gpslc_ctx* c, StreamSlot& s, const TRef& W, const TRef& C, int nt, int ub, int rows) {
    gemm(c, tile_triangle(W, W, C, 0, rows, 0, nt, ub, tri_order(c, rows)), s, 3);
}

// Unit B of a chunk: the full ITE covariance of every pair, W <- D L^-T, CovITE (+ jitter) = Delta - W W^T, and what is asked of
// it: the covariance itself, or draws from it
void unit_b(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nt = sh.nt, L = sh.L;
    const int64_t s0 = ch.s0;
    const TRef W = rect_ref(ch.Wt, (long long)nt * nt * GP_TSQ, nt), Cm = lower_ref(ch.Ct, sh.nlow * GP_TSQ);
    for_pair_batches(sh, ch, [&](int g0, int gs, int l0, int lc, int ub, const TRef& Ls, const TRef& invref) {
        DtArgs da{ch.grid};
        da.s0 = s0 + g0;
        da.lv = io.lv.set(L); da.l0 = l0; da.lc = lc;
        da.pred_noise = io.out.pred_noise; da.W = W; da.Cm = Cm;
        launch_dt_build(da, ub, st);
        w_solve(c, *ch.s, W, Ls, invref, nt, ub, nt);
        minus_w_wt(c, *ch.s, W, Cm, nt, ub, nt);
        if (sh.want_cov) {       // ITEDistributions: single level (lc == 1)
            GatherCovArgs gc{};
            gc.Cm = Cm; gc.n = n; gc.nt = nt; gc.s0 = s0 + g0; gc.S = io.post.S; gc.out = io.CovITEs;
            launch_gather_cov(gc, ub, st);
        }
        if (!sh.want_draws) return;
        // one failure code per pair, then per sample the code of its lowest-index failing level (the reference's loop
        // order, src/prediction.jl:30-33): a shared word per sample would let the lc levels of a diagonal launch race,
        // and the lowest failing tile column win across launches
        HC(hipMemsetAsync(ch.pinfo, 0, sizeof(int) * ub, st));
        factor_robust(c, *ch.s, Cm, nt, ch.pinfo, n, ub, 3);
        launch_fold_pair_info(ch.pinfo, io.info + s0 + g0, gs, lc, st);
        DrawArgs dr{};
        dr.Lc = Cm; dr.n = n; dr.nt = nt; dr.s0 = s0 + g0; dr.S = io.post.S; dr.l = l0; dr.lc = lc; dr.L = L;
        dr.spp = io.out.spp; dr.mean = io.out.meanITE; dr.z = io.out.z; dr.zt = ch.zt; dr.seed = io.out.seed;
        const int64_t eS = io.ens_S > 0 ? io.ens_S : c->ens_S, eo = io.ens_S > 0 ? io.ens_off : c->ens_off;
        dr.rs0 = dr.s0 + (eS > 0 ? eo : 0); dr.rS = eS > 0 ? eS : io.post.S;
        if (L == 1) {     // the reference tensor directly: n x (S*spp), instance fastest
            dr.out = io.out.ite_draws;
            dr.obase = (long long)n * io.out.spp * (s0 + g0); dr.osb = (long long)n * io.out.spp; dr.osl = 0;
            dr.osi = 1; dr.osd = n;
        } else {          // staging [sample][level][d][i]
            dr.out = ch.dtmp;
            dr.obase = (long long)l0 * io.out.spp * n; dr.osb = (long long)L * io.out.spp * n;
            dr.osl = (long long)io.out.spp * n; dr.osi = 1; dr.osd = n;
        }
        {
            ProfScope ps(c, 2, (double)ub * io.out.spp, st);     // unit C: work = draws
            launch_draws(dr, ub, st);
        }
        if (L > 1 && l0 + lc == L)      // the sample group's last levels: its staged draws into the level-fastest tensor
            launch_draws_scatter(ch.dtmp, io.out.ite_draws, n, L, io.out.spp, s0 + g0, gs, st);
    });
}

// Predictions for new individuals of a chunk.  The mean is one pass over the m x n pairs per sample for all
// levels and needs no workspace; variance and covariance batch over (sample, level) pairs like unit B: D*(l) (and prior_l B**)
// into the pair's tiles, W* = D* L^-T against the sample's factor, var from the squared row norms of W*, cov from the lower
// tiles of prior_l B** + pred_noise I - W* W*^T.  Per-individual levels (NewIndividuals::vec) take the mean's pass
// over the pairs and the vector instantiations of the builder and the row norms; the test-set score adds, per pair, the
// factorisation of C in place (the panel schedule, never the persistent launch), the epilogue and the kernel that writes the densities.
void unit_new(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int nt = sh.nt, mt = sh.mt, nb = ch.nb;
    const NewIndividuals& f = io.fresh;
    NewArgs na{};
    static_cast<SampleGrid&>(na) = ch.grid;
    na.Xnew = f.Xnew; na.Unew = f.Unew; na.un_sstride = (long long)f.m * io.nU; na.m = f.m; na.mt = mt;
    na.S = io.post.S; na.lv = io.lv.set(sh.L); na.l0 = 0; na.lc = 1; na.pred_noise = io.out.pred_noise;
    na.alpha = ch.zwork + (long long)nb * sh.Np;
    na.mean = f.mean; na.var = f.var; na.cov = f.cov;
    na.lv.vec = f.vec ? 1 : 0;
    const bool joint = f.lpd_joint != nullptr;
    if (f.score()) { na.noise_s = io.post.p.yNoise; na.Ytest = f.Ytest; na.lpd = f.lpd; na.lpd_joint = f.lpd_joint; na.score = joint ? 1 : 0; }
    if (f.mean) (f.vec ? launch_new_mean_vec : launch_new_mean)(na, nb, st);
    if (sh.new_pairs) {
        na.W = rect_ref(ch.Wt, (long long)mt * nt * GP_TSQ, nt);
        na.Cm = joint ? lower_ref(ch.Ct, (long long)(mt + 1) * (mt + 2) / 2 * GP_TSQ) : f.cov ? lower_ref(ch.Ct, sh.mlow * GP_TSQ) : TRef{};
        for_pair_batches(sh, ch, [&](int g0, int, int l0, int lc, int ub, const TRef& Ls, const TRef& invref) {
            na.s0 = ch.s0 + g0; na.l0 = l0; na.lc = lc;
            launch_new_build(na, ub, st);
            w_solve(c, *ch.s, na.W, Ls, invref, nt, ub, mt);
            launch_new_var(na, ub, st);
            if (f.cov || joint) minus_w_wt(c, *ch.s, na.W, na.Cm, nt, ub, mt);
            if (f.cov) launch_new_gather(na, ub, st);
            if (!f.score()) return;
            if (joint) {      // §28's steps on C: the residual as the one live augmented row, the panel schedule, the epilogue
                launch_new_score_rhs(na, ub, st);
                HC(hipMemsetAsync(ch.pinfo, 0, sizeof(int) * ub, st));
                factor_panels(c, *ch.s, na.Cm, mt, mt + 1, ch.kf_inv, ch.pinfo, 0, ub, 1, true, 3);
                EpiArgs ea{};
                ea.M = na.Cm; ea.n = mt * GP_TS; ea.nt = mt; ea.naug = 1; ea.from_rows = 1;
                ea.logdet = ch.kf_ldq; ea.quad = ch.kf_ldq + ub;       // sample index = batch element: s0 = 0
                launch_epilogue(ea, ub, st);
                na.pinfo = ch.pinfo; na.ldq = ch.kf_ldq;
            }
            launch_new_score_finish(na, ub, st);
        });
    }
    HC(hipGetLastError());
}

}  // namespace

// the chunked ensemble driver (device pointers everywhere)
void run_predict(gpslc_ctx* c, const PredictIO& io_in) {
    PredictIO io = io_in;
    const FormRules& fr = form_rules(io.lv.form);
    const struct { bool refused; const char* why; } refusals[] = {
        {io.lv.vec && !fr.vec, " cannot be combined with vector levels"},
        {(c->flags & GPSLC_FLAG_FP32_KERNEL) && !fr.fp32, " need an fp64 context"},
        {(io.lv.base != nullptr) != fr.baseline, fr.baseline ? " need a baseline" : " cannot be combined with a contrast baseline"}};
    for (const auto& r : refusals)
        if (r.refused) throw std::runtime_error(std::string(fr.name) + r.why);
    if (io.lv.W && io.lv.vec) throw std::runtime_error("weights cannot be combined with vector levels");
    if (io.lv.W && (c->flags & GPSLC_FLAG_FP32_KERNEL)) throw std::runtime_error("weighted effects need an fp64 context");
    if (io.lv.W && io.lv.G < 1) throw std::runtime_error("weights without a weight column");
    if (io.out.covW && (!io.lv.W || !io.out.varSATE)) throw std::runtime_error("the joint covariance needs weights and varW");
    if (io.lv.W && !io.out.meanSATE && !io.out.varSATE) { io.lv.W = nullptr; io.lv.G = 0; }      // nothing weighted is asked for
    if (io.fresh.any()) {
        if (fr.factual) throw std::runtime_error("new individuals have no factual treatment: ordinary levels cannot be predicted for them");
        if (io.lv.vec || io.fresh.m < 1) throw std::runtime_error("new individuals need scalar levels and m >= 1");
        if (io.fresh.cov && !io.fresh.var) throw std::runtime_error("the covariance of new individuals needs their variance: its diagonal");
        if (io.CovITEs || io.out.ite_draws) throw std::runtime_error("new individuals cannot be combined with CovITE or draws: one pair workspace");
        if (io.fresh.vec && io.lv.form != FORM_OUTCOME && io.lv.form != FORM_CONTRAST)
            throw std::runtime_error("per-individual levels of new individuals: outcomes and contrasts only");
        if (io.fresh.score() && (!io.fresh.vec || io.lv.form != FORM_OUTCOME || io.lv.L != 1 || !io.fresh.mean || !io.fresh.var || io.fresh.cov))
            throw std::runtime_error("the test-set score is the outcome form at one per-individual level, with mean and var");
    }
    if (io.fresh.weighted) {
        if (fr.factual) throw std::runtime_error("new individuals have no factual treatment: ordinary levels cannot be predicted for them");
        if (!io.lv.W || io.fresh.m < 1) throw std::runtime_error("weighted averages over new individuals need weights and m >= 1");
        if (io.fresh.any() || io.CovITEs || io.out.ite_draws || io.out.meanITE || io.MeanITEs)
            throw std::runtime_error("weighted averages over new individuals are a call of their own: no per-individual outputs, CovITE or draws");
    }
    if (io.nU < 0) io.nU = c->nU;
    if (io.nX < 0) io.nX = c->nX;
    if (!io.Y) { io.Y = c->dY; io.y_sstride = 0; }
    if (io.post.p.u_sstride == 0 && io.nU > 0 && io.post.p.U != nullptr && !io.p_shared_u) io.post.p.u_sstride = (long long)c->n * io.nU;
    reset_stale_task_timeouts(c);
    ensure_streams(c);
    const PredictShape sh(c, io);
    // chunk size and sub-batch from what the device has (the sub-batch's workspace is sized from the pairs the call
    // really has, and the 30 % rule of the automatic chunk covers its per-sample part only)
    const ChunkBytes by = carve_chunk(sh, io, 0, nullptr);
    // gpslc_y_kfold: the pairs of a sub-batch are (group, sample), a sample has as many as there are large groups
    const int pairs_per_sample = sh.kfold_pairs ? io.lgo.nlarge : sh.L;
    BatchPlan plan;
    try {
        plan = auto_batch(c, io.post.S, pairs_per_sample, by.per_sample, by.per_pair, by.per_level);
    } catch (const std::bad_alloc&) {
        if (!sh.kfold_pairs) throw;
        char buf[200];
        snprintf(buf, sizeof buf, "device workspace allocation failed: group %d has %d members, the workspace of one (group, sample) "
                 "pair is %.1f MB", io.lgo.big_group, io.lgo.big_m, (double)by.per_pair / 1e6);
        throw WorkspaceTooLarge(buf);
    }
    const int Bt = (int)plan.Bt, Bb = (int)plan.Bb;      // Bb: (sample, level) pairs per unit-B sub-batch, no more than the call has
    const size_t need = (size_t)Bt * by.per_sample + plan.fixed;
    for (int i = 0; i < c->nstreams; ++i) c->slots[i].arena.reserve(need);
    // internal MeanITE buffer when the caller did not ask for it but the draws need it
    if (sh.want_draws && !io.out.meanITE) {
        c->scratch.reserve((size_t)sh.n * io.post.S * sh.L * 8 + (1 << 16));
        c->scratch.reset();
        io.out.meanITE = c->scratch.take<double>((size_t)sh.n * io.post.S * sh.L);
    }
    HC(hipMemsetAsync(io.info, 0, sizeof(int) * io.post.S, c->slots[0].st));
    HC(hipStreamSynchronize(c->slots[0].st));
    int chunk = 0;
    for (int64_t s0 = 0; s0 < io.post.S; s0 += Bt, ++chunk) {
        Chunk ch{&c->slots[chunk % c->nstreams], s0, (int)std::min<int64_t>(Bt, io.post.S - s0)};
        ch.s->arena.reset();
        carve_chunk(sh, io, Bb, &ch);
        ch.grid = SampleGrid{io.X, c->dT, io.post.p, s0, sh.n, io.nX, io.nU, sh.nt};
        const bool back_done = unit_a(c, io, sh, ch);
        if (sh.want_alpha && !back_done) back_substitute(sh, ch);
        if (sh.want_mean) mean_ite(c, io, sh, ch);
        if (sh.want_w) loo(io, sh, ch);
        if (sh.kfold_pairs) kfold_large(c, io, sh, ch);
        if (sh.want_grad) grad(io, sh, ch);
        if (sh.unitB) unit_b(c, io, sh, ch);
        if (sh.want_new) unit_new(c, io, sh, ch);
    }
    for (auto& s : c->slots) HC(hipStreamSynchronize(s.st));
    HC(hipGetLastError());
    check_task_timeout(c);
    if (c->flags & GPSLC_FLAG_PROFILE) prof_collect(c);
    c->last_info.resize(io.post.S);
    HC(hipMemcpy(c->last_info.data(), io.info, sizeof(int) * io.post.S, hipMemcpyDeviceToHost));
}

}  // namespace gpslc_host
