// A prediction call as run_predict takes it (device pointers everywhere): the posterior samples, the levels, the outputs, and
// what the outcome-model and new-individual calls add.  The chunk loop behind run_predict (predict.hip) uses the schedules of
// factor.h; it knows nothing of host pointers, argument positions or entry points.
#pragma once
#include "factor.h"

namespace gpslc_host {

// One prediction call is described once, by three pieces: the extern "C" entry points fill them with the caller's pointers
// (PredictRequest: host or device, as given) and run_predict reads them with device pointers (PredictIO).
struct Posterior {                   // the S posterior samples of the call
    int64_t S = 0;
    SampleParams p{};                // the six per-sample arrays
};
// What each level form (level_form.h) can be combined with: run_predict's backstop behind the entry points' validate.  A baseline
// is required by the paired form and refused by the others.  Every form takes weights: their rules stay in run_predict.
struct FormRules { int form; const char* name; bool factual, baseline, vec, fp32; };
template <int FORM, typename LF = LevelForm<FORM>>
constexpr FormRules form_row(const char* name) { return {FORM, name, LF::factual, LF::paired, LF::vector_levels, LF::fp32_kernels}; }
constexpr FormRules kFormRules[] = {form_row<FORM_ORDINARY>("ordinary levels"), form_row<FORM_CONTRAST>("contrasts"),
                                    form_row<FORM_SLOPE>("slopes"), form_row<FORM_OUTCOME>("outcomes")};
static const FormRules& form_rules(int form) {
    for (const FormRules& r : kFormRules)
        if (r.form == form) return r;
    throw std::runtime_error("unknown level form");
}

struct Levels {
    int L = 0;
    const double* doT = nullptr;
    bool vec = false;                // vector levels: doT is n x L (level l at doT + n*l), not L scalars
    int form = FORM_ORDINARY;        // FORM_* (level_form.h), set by the entry points
    const double* base = nullptr;    // FORM_CONTRAST (L): level l is doT[l] against base[l]
    void against(const double* b) { base = b; form = b ? FORM_CONTRAST : FORM_ORDINARY; }   // a contrast exactly when a baseline is given
    bool needs_kw() const { return form_rules(form).factual; }     // only the factual term brings K W in
    LevelSet set(int nlevels) const { return LevelSet{doT, base, nlevels, form, vec ? 1 : 0}; }      // what the kernels take
    // weighted effects: G weight columns — the caller's W[i + n*g] on the host, column fastest (W[g + G*j]) on the
    // device; meanSATE / varSATE are then S x L x G — element (s, l, g) at s + S*(l + L*g) — of tau_w = w_g' ITE_l, the weights
    // used as given (scalar levels only)
    int G = 0;
    const double* W = nullptr;
};
struct DrawsAndOutputs {
    double pred_noise = 0;
    int spp = 0;
    uint64_t seed = 0;
    const double* z = nullptr;
    double *meanSATE = nullptr, *varSATE = nullptr, *meanITE = nullptr, *ite_draws = nullptr;
    // weighted calls only: the joint covariance of the L levels per weight column, S x L x L x G — element
    // (s, l, l', g) at s + S*(l + L*(l' + L*g)); needs varSATE, whose values are its diagonal
    double* covW = nullptr;
};

// What the outcome-model calls add to a prediction call: device pointers, null where the output is not asked
struct Loo {                         // leave-one-out predictive checks (gpslc_y_loo): n x S each
    double *mean = nullptr, *var = nullptr, *lpd = nullptr;
    bool any() const { return mean || var || lpd; }
};
struct Lgo {                         // leave-group-out predictive checks (gpslc_y_lgo): n x S, n x S, G x S
    int G = 0, mmax = 0;             // groups; members of the largest
    const int *members = nullptr, *offsets = nullptr;      // the members sorted by (group, row), the G + 1 offsets into them
    double *mean = nullptr, *var = nullptr, *lpd = nullptr;
    bool any() const { return mean || var || lpd; }
    // gpslc_y_kfold (kfold == false: every group goes through lgo_group_kernel, gpslc_y_lgo's launch).  The groups
    // of at most LGO_MAX_GROUP members are the nsmall entries of `split` (mmax: the largest of THEM), the larger ones follow in
    // classes of equal tile count mt = ceil(m / 128): the batch elements of the tiled path's launches share it
    struct Class { int mt, first, count; };     // `count` groups from split[first] on
    bool kfold = false;
    const int* split = nullptr;                 // device: group numbers, the small ones first, then class by class
    int nsmall = 0, nlarge = 0;
    std::vector<Class> classes;
    int big_group = 0, big_m = 0;               // the largest group and its size: named when its workspace does not fit
    int mt_max() const { return classes.empty() ? 0 : classes.back().mt; }      // ascending mt
};
struct Grad {                        // gradient of the outcome log-likelihood (gpslc_y_logpdf_grad), in the layouts of
    // the arguments they differentiate: U n x nU x S, uyLS nU x S, xyLS nX x S, the others S; Y n x S
    double *U = nullptr, *uyLS = nullptr, *xyLS = nullptr, *tyLS = nullptr, *yScale = nullptr, *yNoise = nullptr, *Y = nullptr;
    bool pairs() const { return U || uyLS || xyLS || tyLS; }     // those that need the pass over the pairs
    bool needs_c() const { return yScale || yNoise; }            // those that need c = diag(A^-1)
    bool any() const { return pairs() || needs_c() || Y; }
};
struct NewIndividuals {              // predictions for m new individuals (gpslc_predict_new)
    const double *Xnew = nullptr, *Unew = nullptr;      // their features: m x nX, m x nU x S
    int m = 0;
    double *mean = nullptr, *var = nullptr, *cov = nullptr;     // m x S x L each and m x m x S x L; cov needs var: its diagonal
    // per-individual levels (gpslc_predict_new_vec): Levels::doT / base are m x L over the NEW individuals (level l
    // of new individual i at doT[i + m*l]); Levels::vec stays false, it speaks of the n training individuals
    bool vec = false;
    // the test-set score (gpslc_y_test): the outcome form with vec, L = 1, doT = the test set's treatments and yNoise for
    // pred_noise; mean and var are always there, lpd (m x S) and lpd_joint (S) may be null
    const double* Ytest = nullptr;
    double *lpd = nullptr, *lpd_joint = nullptr;
    bool score() const { return Ytest != nullptr; }
    bool pairs() const { return var || cov; }            // the (sample, level) pairs need tile workspace
    bool any() const { return mean || pairs(); }
    // weighted averages over them (gpslc_predict_new_weighted), a call of its own: Levels::W / G are then G weight
    // columns over the m NEW individuals (device: W[g + G*i]) and DrawsAndOutputs::meanSATE / varSATE / covW receive meanW, varW, covW
    bool weighted = false;
};

struct PredictIO {
    Posterior post;
    Levels lv;
    DrawsAndOutputs out;
    const double* X = nullptr;   // device X to use (ctx or override)
    double *logdet = nullptr, *quad = nullptr;
    // ITEDistributions-style outputs (single level): MeanITEs S x n, CovITEs S x n x n
    double *MeanITEs = nullptr, *CovITEs = nullptr;
    int* info = nullptr;   // device, S
    int nU = -1, nX = -1;            // feature counts of this call (default: the ctx's)
    const double* Y = nullptr;       // right-hand side 0 (default: the ctx's Y) and its per-sample stride
    long long y_sstride = 0;
    bool p_shared_u = false;         // the feature block is shared by all samples (u_sstride stays 0)
    int64_t ens_off = 0, ens_S = 0;  // ens_S > 0: this call's placement in a larger ensemble (else the ctx's, gpslc_set_ensemble)
    // node draws (gpslc_nodes_draw beyond the single-workgroup kernels): ndraw[:, s] = chol(A_s) nz[:, s] from the batched
    // tiled factor of A_s (n x S each, device; nzero = n x S zeros, the draw kernel's mean)
    const double* nz = nullptr;
    const double* nzero = nullptr;
    double* ndraw = nullptr;
    Loo loo;
    Lgo lgo;
    Grad grad;
    bool grad_no_t = false;          // node mode of the gradient (GradArgs::no_t): no treatment column
    NewIndividuals fresh;
};

void run_predict(gpslc_ctx* c, const PredictIO& io_in);
DrawArgs zero_mean_draw(TRef Lc, int n, int nt, long long s0, long long S, const double* zero, const double* z, double* zt,
                        double* out);
void w_solve(gpslc_ctx* c, StreamSlot& s, const TRef& W, const TRef& Ls, const TRef& invref, int nt, int ub, int rows);

}  // namespace gpslc_host
