/*
 * gpslc_hip.h — C ABI of libgpslc_hip.so, the MI355X (gfx950) implementation of the
 * CausalGPSLC.jl GP-kernel + posterior-prediction hot path.
 *
 * Every entry point replaces the body of one Julia function of the reference (cited per
 * function, paths relative to the reference repository).  The Julia side keeps its
 * signatures and `ccall`s these (INTEGRATION.md shows the shim); in this repository a
 * Python ctypes harness (causalgpslc.jl_amd/_lib.py) binds exactly the same symbols.
 *
 * Conventions
 *   - all matrices are COLUMN-MAJOR (Julia layout), all reals are IEEE double;
 *   - Bool treatments are pre-converted by the caller to 0.0 / 1.0 (Julia promotes Bool on
 *     subtraction, src/kernel.jl:17);
 *   - return value: 0 = ok; < 0 = error (GPSLC_ERR_*; -1..-99 = "argument #k is invalid");
 *     > 0 = 1-based index of the pivot at which a Cholesky factorisation broke down
 *     (the Julia shim rethrows it as PosDefException(info), mirroring PDMats);
 *   - no C++ exception, abort or longjmp crosses this boundary;
 *   - the caller owns every host/device buffer it passes; the library keeps no pointer to
 *     caller memory after a call returns; device workspace belongs to the ctx;
 *   - calls on one ctx must be serialised by the caller; use one ctx per GPU / per thread.
 *   - "_dev" variants take DEVICE pointers (hipMalloc'ed / torch / AMDGPU.jl memory on the
 *     ctx's device) for every array argument; the plain variants take HOST pointers.
 *   - stream contract of the "_dev" variants: the library works on private non-blocking HIP streams of
 *     the ctx.  The caller must have completed (synchronised) whatever produced its device inputs
 *     before the call; when the call returns every output is complete and visible to any stream.
 *   - thread safety: distinct ctxs may be used concurrently from distinct threads (also on the same
 *     GPU); the library keeps no process-global mutable state besides per-device "attribute applied"
 *     bits, which are atomic.  The environment is never consulted by this library.
 */
#ifndef GPSLC_HIP_H
#define GPSLC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpslc_ctx gpslc_ctx;

#define GPSLC_OK                 0
#define GPSLC_ERR_HIP        (-1000)  /* a HIP runtime call failed; see gpslc_last_error  */
#define GPSLC_ERR_NOMEM      (-1001)  /* device workspace could not be allocated          */
#define GPSLC_ERR_NODATA     (-1002)  /* gpslc_set_data has not been called               */
#define GPSLC_ERR_NODEVICE   (-1003)  /* no usable gfx950 device                          */
#define GPSLC_ERR_INTERNAL   (-1004)
#define GPSLC_ERR_IO         (-1005)  /* posterior pack: file cannot be opened / read / written   */
#define GPSLC_ERR_FORMAT     (-1006)  /* posterior pack: bad magic, truncated or trailing bytes   */
#define GPSLC_ERR_UNSUPPORTED (-1007) /* the entry point does not cover this problem size / mode  */

/* flags for gpslc_create */
#define GPSLC_FLAG_DEFAULT            0u
#define GPSLC_FLAG_PROFILE            1u   /* record HIP events around the dominant kernels */
#define GPSLC_FLAG_FP32_KERNEL        2u   /* mixed precision (BASELINE config 5): RBF distances and exp in
                                              fp32, Gram matrix / Cholesky / solves in fp64; features centred
                                              per column before rounding (the answer does not depend on where
                                              the data's origin is)                                          */

/* ---- context ------------------------------------------------------------------------- */

/* One context per (GPU, data set).  n = instances, nX = covariate columns (0 = model without
 * X), nU = latent confounder columns (0 = model without U).  Plays the role of the data part
 * of GPSLCObject (src/types.jl:249-258). */
int gpslc_create(gpslc_ctx** out, int device, int64_t n, int32_t nX, int32_t nU, uint32_t flags);
int gpslc_destroy(gpslc_ctx* ctx);

/* g.X (n x nX, may be NULL when nX == 0), g.T (n), g.Y (n): src/types.jl:249-258.  The arrays are copied; the caller
 * may free or reuse its arrays after the call (host pointers, or device pointers for _dev). */
int gpslc_set_data(gpslc_ctx* ctx, const double* X, const double* T, const double* Y);
int gpslc_set_data_dev(gpslc_ctx* ctx, const double* X, const double* T, const double* Y);

/* Tuning knobs (0 = keep default): max posterior samples factorised concurrently, tile-panel
 * width of the blocked Cholesky, number of HIP streams chunks are spread over.  A panel width given here
 * also bounds the persistent task launch (gpslc_set_task_schedule below): matrices of more tiles per side
 * than panel_tiles then take the panel schedule (left-looking panels + trailing updates) instead of
 * being factorised as ONE panel of tasks. */
int gpslc_set_tuning(gpslc_ctx* ctx, int32_t max_batch, int32_t panel_tiles, int32_t n_streams);

/* Schedule of the factorisation of A at small tile counts (round 6; no reference counterpart: the reference factorises
 * one matrix at a time, src/likelihood.jl:42-43, src/estimation.jl:46).  Chunks of at least min_matrices matrices of
 * min_tiles .. max_tiles tiles of 128 per side (and at most panel_tiles wide: one left-looking panel) are factorised — and,
 * where MeanITE is wanted, back-substituted (src/estimation.jl:46's CovWWp \ Y) — by ONE persistent launch of tile tasks:
 * diagonal-tile, strip and back-substitution tasks of many matrices in flight at once, dependencies through per-matrix
 * progress words, instead of one launch per tile column.  Every output is bit-identical either way.
 * min_tiles: <= 0 = keep (default 2: N > 128); max_tiles: 0 = always one launch per column, negative = keep (default and
 * limit 32: N <= 4096 — beyond that, and beyond one panel of gpslc_set_tuning's panel_tiles when that was given, the panel
 * schedule is kept: left-looking panels of per-column launches + one trailing update per panel); min_matrices: <= 0 = keep (default 256: a persistent launch
 * over a few matrices is a chain of hand-offs — the single scores of an MH step keep the per-column launches); group:
 * matrices per group of the task order, <= 0 = keep (default 32).  Returns 0, or minus the number of the offending argument. */
int gpslc_set_task_schedule(gpslc_ctx* ctx, int32_t min_tiles, int32_t max_tiles, int32_t min_matrices, int32_t group);

/* Placement of a call's posterior samples inside a larger ensemble, for the library's own normals (z_or_null == NULL):
 * after gpslc_set_ensemble(ctx, s_off, S_total) sample s, level l of gpslc_predict[_dev] draws from the Philox stream
 * (s_off + s) + S_total * l instead of s + S * l.  A rank of a sharded prediction that holds the samples [s0, s1) of
 * S_total (the partition of the loop src/estimation.jl:78-84 under src/prediction.jl:30-33) sets (s0, S_total) and then
 * generates exactly the normals a single-process call over all S_total samples generates for them — the result does not
 * depend on the number of ranks.  S_total = 0 restores the default (offset 0, the call's own S). */
int gpslc_set_ensemble(gpslc_ctx* ctx, int64_t sample_offset, int64_t S_total);

const char* gpslc_last_error(const gpslc_ctx* ctx);

/* ---- src/kernel.jl ------------------------------------------------------------------- */

/* rbfKernelLog(X1, X2, LS) (src/kernel.jl:24-32; vectors are d = 1):
 * out[i + n*ip] = -sum_k (X1[i,k] - X2[ip,k])^2 / LS[k]^2, ls_len = 1 (scalar LS) or d. */
int gpslc_rbf_log(gpslc_ctx* ctx, const double* X1, const double* X2, int64_t n, int32_t d,
                  const double* ls, int32_t ls_len, double* out);
/* device pointers for X1, X2, ls and out: no allocation, no copy (src/inference.jl:225-227, 286-287, 343-344
 * call rbfKernelLog / processCov once per outer MCMC iteration) */
int gpslc_rbf_log_dev(gpslc_ctx* ctx, const double* X1, const double* X2, int64_t n, int32_t d,
                      const double* ls, int32_t ls_len, double* out);

/* processCov(logCov, scale[, noise]) (src/kernel.jl:53-55, 57-59): out = exp.(logcov)*scale
 * + noise*I.  The two-argument method is noise = 0.0. */
int gpslc_process_cov(gpslc_ctx* ctx, const double* logcov, int64_t n, double scale, double noise,
                      double* out);
int gpslc_process_cov_dev(gpslc_ctx* ctx, const double* logcov, int64_t n, double scale, double noise,
                          double* out);   /* device pointers; out may alias logcov */

/* ---- src/model_likelihood.jl :Y node -------------------------------------------------- */

/* logpdf(MvNormal(0, Symmetric(Ycov)), Y) with Ycov = processCov(uyCovLog .+ xyCovLog .+
 * tyCovLog, yScale, yNoise): generateYfromUXT / UT / XT / T (src/model_likelihood.jl:83-91,
 * 94-101, 104-111, 114-120).  U: n x nU (ignored when nU == 0).  X_or_null: overrides the ctx's
 * X for this call (the trace's :X => k => :X values; n x nX) or NULL to use gpslc_set_data's.
 * Y_or_null: the value being scored (n) — what Gen hands to a Distribution's logpdf — or NULL for
 * the ctx's Y (the constrained observation, src/model_likelihood.jl:89).  Uses the ctx's T.
 * S independent parameter sets are evaluated per call (S = 1 for one Gen `update`); U is
 * n x nU x S, uyLS nU x S, xyLS nX x S, the rest length S. */
int gpslc_y_logpdf(gpslc_ctx* ctx, int64_t S, const double* U, const double* X_or_null,
                   const double* Y_or_null, const double* uyLS, const double* xyLS, const double* tyLS,
                   const double* yScale, const double* yNoise, double* logpdf /* S */);

/* Leave-one-out (LOO) predictive checks of the outcome model Y ~ N(0, A), A = Ycov as above = L L^T (Rasmussen &
 * Williams, Gaussian Processes for Machine Learning, §5.4.2).  With alpha = A^-1 Y and c_i = [A^-1]_ii, for every individual
 * i and parameter set s (element (i, s) of an n x S array at i + n*s):
 *   looMean = Y_i - alpha_i / c_i                                   mean of Y_i given all the other observations
 *   looVar  = 1 / c_i                                               its variance: predictive for the OBSERVATION, yNoise included
 *   looLpd  = -log(2 pi)/2 + log(c_i)/2 - alpha_i^2 / (2 c_i)       log density of Y_i under that predictive
 * c is computed as the squared row norms of L^-T from the tiled factor (a sum of squares: no cancellation), on the GPU.
 * Each parameter set's LOO conditions on THAT set's hyper-parameters and U, which were themselves inferred with Y_i present:
 * it checks the outcome surface given the posterior sample, not the whole inference (no importance-weighting correction).
 * Arguments as gpslc_y_logpdf (host pointers; X_or_null / Y_or_null override the ctx's X / Y for this call).  Any of the four
 * outputs may be NULL; all four NULL is the argument error of looMean (-11).  logpdf_or_null receives gpslc_y_logpdf's value
 * from the same factorisation: bit-identical to that call wherever it takes the batched tiled path (n > 640, more
 * parameter sets than the single-launch kernels take, or a GPSLC_FLAG_FP32_KERNEL context) — this call takes the tiled path
 * at every n.  Works on any context (nothing here evaluates the RBF kernel beyond the shared Gram build).
 * A parameter set whose factorisation breaks down gets NaN in all its LOO outputs; return value (first failing pivot) and
 * gpslc_last_info as for gpslc_y_logpdf.  There is no _dev variant and no sharding over several contexts. */
int gpslc_y_loo(gpslc_ctx* ctx, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                double* looMean /* n x S */, double* looVar /* n x S */, double* looLpd /* n x S */,
                double* logpdf_or_null /* S */);

/* Leave-group-out (LGO) predictive checks of the same outcome model: a whole group of individuals (the members of an object;
 * a cross-validation fold) is removed and predicted jointly from everybody else.  labels[i] in [0, G) is the group of
 * individual i; every group has at least one member and at most 128.  For a group I of m members, alpha = A^-1 Y and
 * C = [A^-1]_II (Rasmussen & Williams §5.4.2 in block form), for every parameter set s:
 *   lgoMean[i + n*s] = [Y_I - C^-1 alpha_I]_i         mean of Y_i given every individual outside i's group
 *   lgoVar[i + n*s]  = [C^-1]_ii                      its marginal variance: for the OBSERVATION, yNoise included
 *   lgoLpd[g + G*s]  = -(m/2) log(2 pi) + log det(C)/2 - alpha_I^T C^-1 alpha_I / 2      joint log density of the whole group
 * C is a Gram matrix of rows of L^-T from the tiled factor (a sum of products, no subtraction from a prior term), factorised
 * C = R R^T in the workgroup's local memory; lgoVar is the squared norm of a column of R^-1, a sum of squares.
 * Arguments 1-10, validation, overrides and logpdf_or_null are gpslc_y_loo's (logpdf_or_null is bit-identical to that call's);
 * works on a GPSLC_FLAG_FP32_KERNEL context.  Any output may be NULL.  Errors: G < 1 or G > n: -11; labels NULL, a label
 * outside [0, G) or a group without a member: -12; lgoMean, lgoVar and lgoLpd all NULL: -13; a group of more than 128 members:
 * GPSLC_ERR_UNSUPPORTED, gpslc_last_error names the group and its size (larger groups need the tiled factorisation of C:
 * gpslc_y_kfold below).  S = 0 is an empty call.
 * A parameter set whose factorisation of A breaks down gets NaN in all its outputs; return value (first failing pivot) and
 * gpslc_last_info as for gpslc_y_loo.  A group whose C loses positive definiteness in the small factorisation gets NaN in its
 * outputs for that parameter set; the return value and gpslc_last_info do not change.
 * Guarantees: the outputs are bit-reproducible and independent of chunking, stream count and factorisation schedule.  A
 * group's outputs depend only on its member set, the members taken in ascending row order: not on its label number, not on
 * how the other individuals are grouped.  Groups of one member give gpslc_y_loo's values to rounding (the summation order
 * differs); one group of everybody (n <= 128) gives lgoLpd = logpdf, lgoMean = 0 (the prior mean) and lgoVar = diag(A), to
 * rounding.  There is no _dev variant, no sharding over several contexts and no joint covariance output. */
int gpslc_y_lgo(gpslc_ctx* ctx, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                int32_t G, const int32_t* labels /* n, values in [0, G) */,
                double* lgoMean /* n x S */, double* lgoVar /* n x S */, double* lgoLpd /* G x S */,
                double* logpdf_or_null /* S */);

/* K-fold cross-validation of the same outcome model: gpslc_y_lgo for groups of ANY size, 1 .. n members — 5 or 10 folds at any
 * n, a hospital of 129 patients.  Signature, argument numbering, validation order, overrides, logpdf_or_null, outputs, layouts
 * and the errors -11 / -12 / -13 are gpslc_y_lgo's; works on a GPSLC_FLAG_FP32_KERNEL context.
 * Groups of at most 128 members go through gpslc_y_lgo's kernel: a call whose groups are all that small returns that call's
 * outputs bit for bit.  For a larger group, C = [A^-1]_II is built as 128 x 128 tiles in device memory (mt = ceil(m / 128) tile
 * rows) with alpha_I beside it, and factorised, solved with and inverted on its diagonal by the kernels that do the same for A:
 * cvMean = Y_I - C^-1 alpha_I, cvVar = diag(C^-1) as squared row norms of C's own L^-T, cvLpd from log det C and the quadratic
 * form.  The (group, sample) pairs of the larger groups run in sub-batches whose workspace (about (mt^2 + 3 mt) x 128 KiB per pair)
 * is sized from the free device memory; a call in which not even one pair fits returns GPSLC_ERR_NOMEM, before any launch, and
 * gpslc_last_error names the largest group and its size.
 * A parameter set whose factorisation of A breaks down gets NaN in all its outputs; return value and gpslc_last_info as for
 * gpslc_y_lgo.  A group whose C loses positive definiteness gets NaN for that parameter set; the return value and
 * gpslc_last_info do not change.
 * Guarantees, for groups of every size: the outputs are bit-reproducible and independent of chunking, stream count, sub-batching
 * of the pairs and factorisation schedule; a group's outputs depend only on its member set, the members taken in ascending row
 * order: not on its label number, not on how the other individuals are grouped.  One group of everybody gives cvLpd = logpdf,
 * cvMean = 0 and cvVar = diag(A), to rounding, at any n.  Nothing is continuous in the bits across m = 128 / 129: the two paths
 * sum in different orders.  There is no _dev variant, no sharding over several contexts and no joint covariance output. */
int gpslc_y_kfold(gpslc_ctx* ctx, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                  const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                  int32_t G, const int32_t* labels /* n, values in [0, G) */,
                  double* cvMean /* n x S */, double* cvVar /* n x S */, double* cvLpd /* G x S */,
                  double* logpdf_or_null /* S */);

/* Gradient of the :Y node's score log N(Y; 0, A), A = K + yNoise I, K_ij = yScale exp(-sum_f ((w_if - w_jf) / ls_f)^2) over
 * the features w = [U | X | T] with ls = [uyLS; xyLS; tyLS], for S parameter sets: what a gradient-based move on U and the
 * hyper-parameters (HMC, MALA, MAP), a type-II maximum-likelihood start or a sensitivity check needs (Rasmussen & Williams
 * §5.4.1).  With alpha = A^-1 Y, Q = alpha alpha^T - A^-1, P = Q o K (element-wise), c = diag(A^-1) and D_ijf = w_if - w_jf:
 *   dLS_f    =  (1 / ls_f^3) sum_ij P_ij D_ijf^2                    every feature: duyLS (nU x S), dxyLS (nX x S), dtyLS (S)
 *   dU_if    = -(2 / ls_f^2) sum_j P_ij D_ijf                       f < nU: dU (n x nU x S)
 *   dyNoise  =  (alpha . alpha - sum_i c_i) / 2                     (S)
 *   dyScale  =  (alpha . Y - n - yNoise (alpha . alpha - sum_i c_i)) / (2 yScale)        (S)
 *   dY       = -alpha                                               (n x S)
 * Every output has the layout of the argument it differentiates (dU: element (i, f, s) at i + n*(f + nU*s)).  A^-1 is formed
 * tile by tile from the L^-T of gpslc_y_loo on the f64 matrix cores and never stored; K is evaluated again in fp64 and D from
 * the raw features; c is a sum of squares.  Derivatives are with respect to the parameters themselves, not their logarithms.
 * Arguments 1-10, validation, overrides and logpdf_or_null are gpslc_y_loo's (logpdf_or_null is bit-identical to that call's);
 * this call takes the tiled path at every n.  Any output may be NULL; dU .. dY all NULL is the argument error of dU (-11).
 * With nU == 0 (nX == 0) the outputs of that block are ignored.  When only dyScale, dyNoise and dY are asked for, no pass over
 * the pairs runs and the call costs what gpslc_y_loo costs.  A GPSLC_FLAG_FP32_KERNEL context: GPSLC_ERR_UNSUPPORTED (the
 * fp64 K of the pair pass is not the matrix such a context factorises).  S = 0 is an empty call.
 * A parameter set whose factorisation breaks down gets NaN in all its outputs; return value (first failing pivot) and
 * gpslc_last_info as for gpslc_y_loo.
 * Guarantees: the outputs are bit-reproducible and independent of chunking, stream count and factorisation schedule (no
 * floating-point atomics: fixed summation orders); asking for a subset of the outputs gives the same bits for that subset;
 * sum_i dU[i, f, s] vanishes to rounding (the score does not change when a column of U is shifted).
 * There is no _dev variant and no sharding over several contexts; no gradient with respect to X or T. */
int gpslc_y_logpdf_grad(gpslc_ctx* ctx, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                        const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                        double* dU /* n x nU x S */, double* duyLS /* nU x S */, double* dxyLS /* nX x S */,
                        double* dtyLS /* S */, double* dyScale /* S */, double* dyNoise /* S */, double* dY /* n x S */,
                        double* logpdf_or_null /* S */);

/* ---- the other Gaussian-process nodes of the Gen models -------------- */

/* log N(target; 0, scale * exp.(rbfKernelLog(F, F, ls)) + noise * I) for S parameter sets: the score of
 *   :X => k => :X   generateXfromU    F = U,       ls = uxLS[k, :]           (src/model_likelihood.jl:13-22)
 *   :T / :logitT    generate*TfromUX  F = [U | X], ls = [utLS ; xtLS]        (src/model_likelihood.jl:25-80)
 *   :Y              generateYfrom*    F = [U | X | T]                        (:83-120; gpslc_y_logpdf is the
 *                                                                             specialised form that shares X, T, Y)
 * F is n x nF x S (f_shared = 0) or n x nF shared by all sets (f_shared = 1); ls nF x S; scale, noise S;
 * target n x S (t_shared = 0) or n (t_shared = 1).  nF <= 32. */
int gpslc_gp_logpdf(gpslc_ctx* ctx, int64_t S, int32_t nF, const double* F, int32_t f_shared,
                    const double* ls, const double* scale, const double* noise, const double* target,
                    int32_t t_shared, double* logpdf /* S */);

/* The fused whole-model score: `count` independent Gaussian-process nodes, each with its OWN feature block, in one
 * call — what one Gen `update` re-scores (src/model.jl:11-131): the nX `:X => k => :X` nodes, `:T` / `:logitT` and
 * `:Y` (F = [U | X | T], ls = [uyLS ; xyLS ; tyLS]) of a proposal, or the nodes of several proposals at once.
 * logpdf[i] = log N(target_i; 0, scale_i * exp.(rbfKernelLog(F_i, F_i, ls_i)) + noise_i * I); host pointers.
 * While the n x n matrix fits one CU's LDS (n <= 160 for any nF <= 32, up to n = 176 for nF <= 16) ALL nodes are
 * scored by ONE kernel launch, one workgroup per node (Gram build, Cholesky, forward solve and reductions never
 * leave the CU); gpslc_gp_logpdf and gpslc_y_logpdf take the same path at those sizes.  Larger n: ONE batched pass of
 * the general tiled path over all nodes (feature blocks zero-padded to the widest node with lengthscale-1 columns, which
 * add +0.0 to every squared distance: scores bit-identical to node-by-node calls; 3 nodes cost 1.09 x one at n = 4096).
 * Return value and gpslc_last_info (count entries) as for gpslc_gp_logpdf. */
typedef struct gpslc_node {
    int32_t nF;            /* feature columns, 0..32 */
    int32_t reserved;
    const double* F;       /* n x nF, column-major */
    const double* ls;      /* nF */
    double scale, noise;
    const double* target;  /* n */
} gpslc_node;
int gpslc_nodes_logpdf(gpslc_ctx* ctx, int32_t count, const gpslc_node* nodes, double* logpdf /* count */);

/* The fused whole-model gradient: the gradient of every score of gpslc_nodes_logpdf in one call — what a gradient-based move on
 * a latent confounder (HMC, MALA, MAP) needs, since U feeds every `:X => k => :X` node, `:T` / `:logitT` and `:Y`.  Node i is
 * that of gpslc_nodes_logpdf: its score is log N(target_i; 0, A_i), A_i = K_i + noise_i I, K_i = scale_i exp(-sum_f ((F_rf -
 * F_cf) / ls_f)^2).  With alpha = A^-1 target, Q = alpha alpha^T - A^-1, P = Q o K, c = diag(A^-1), D_rcf = F_rf - F_cf:
 *   dF_rf    = -(2 / ls_f^2) sum_c P_rc D_rcf                 EVERY feature column of the node
 *   dls_f    =  (1 / ls_f^3) sum_rc P_rc D_rcf^2
 *   dnoise   =  (alpha . alpha - sum_r c_r) / 2
 *   dscale   =  (alpha . target - n - noise (alpha . alpha - sum_r c_r)) / (2 scale)
 *   dtarget  = -alpha
 * with respect to the parameters themselves, not their logarithms.  Layouts (host; flat, no struct): dF is the nodes' n x nF_i
 * column-major blocks concatenated in node order (node i starts at n sum_{k<i} nF_k), dls the same with nF_i values per node;
 * dscale, dnoise and logpdf_or_null hold `count` values; dtarget is n x count.  A node with nF = 0 owns no slot of dF / dls.
 * Any of arguments 4-9 may be NULL; 4-8 all NULL returns -4; count < 0: -2; nodes NULL or a malformed node: -3; count = 0 is
 * an empty call.  A GPSLC_FLAG_FP32_KERNEL context: GPSLC_ERR_UNSUPPORTED.  Needs no gpslc_set_data.  A node whose factorisation
 * breaks down gets NaN in all its gradient outputs; the call returns the first failing pivot, gpslc_last_info has count entries.
 * Paths: while every node fits one CU's LDS with the gradient's extra image (the score's packed blocks, the scaled AND the raw
 * features, alpha) and count <= 4096, ONE launch, one workgroup per node: the score kernel's own Gram build and Cholesky, then
 * L^-1, A^-1 = L^-T L^-1 and P in place in LDS on the f64 matrix cores and the sums over the pairs, D from the raw features.
 * Largest n of that path per widest node of the call:
 *     nF <= 7: 176      nF <= 17: 160      nF <= 27: 144      nF <= 32: 128
 * Otherwise the whole call takes the batched tiled path: gpslc_y_logpdf_grad's pair pass without a treatment column over the
 * nodes padded to the widest one; the padding columns' gradients are dropped.  (The left-looking kernel that scores
 * 176 < n <= 640 has no gradient mode.)
 * Guarantees: the outputs are bit-reproducible from run to run (no floating-point atomics, fixed summation orders); on a given
 * path a node's outputs do not depend on which other nodes share the call, on the widest of them, or on the node's position;
 * asking for a subset of the outputs gives the same bits for that subset; sum_r dF[r, f] vanishes to rounding; logpdf_or_null is
 * bit-identical to gpslc_nodes_logpdf for the same nodes whenever both calls take the same path (they differ where the score
 * fits its single launch and the gradient's larger image does not).  No _dev variant; dense-covariance (`:U` prior) nodes have
 * no node kind here: their gradient -Sigma^-1 x / covscale is one solve with gpslc_mvn_logpdf's cached factor.   */
int gpslc_nodes_logpdf_grad(gpslc_ctx* ctx, int32_t count, const gpslc_node* nodes, double* dF /* n x sum nF */,
                            double* dls /* sum nF */, double* dscale /* count */, double* dnoise /* count */,
                            double* dtarget /* n x count */, double* logpdf_or_null /* count */);

/* Draws from the nodes' priors: draws[:, i] = chol(K_i) * target_i with K_i the node's covariance as above and
 * target_i a vector of standard normals supplied by the caller (the host keeps its random-number stream) — what Gen's
 * `mvnormal(zeros(n), cov)` does inside `elliptical_slice(trace, addr, mu, cov)` (src/inference.jl:48-54, 92-98, 232,
 * 348; covariances built at src/inference.jl:225-227, 286-287, 343-344) and inside `generate` for the prior draws.
 * Same single launch as gpslc_nodes_logpdf while the single-workgroup kernels cover the call (n <= 640, count <= 512: the
 * factor never leaves the CU / its L2 scratch); beyond — larger n, more nodes, the fp32 kernel mode — the batched tiled
 * factorisation of every node's covariance followed by L z on the predictive-draw kernel (round 6).  logpdf_or_null, when
 * given, receives log N(target_i; 0, K_i) as a by-product.  Return value / gpslc_last_info as above. */
int gpslc_nodes_draw(gpslc_ctx* ctx, int32_t count, const gpslc_node* nodes, double* draws /* n x count */,
                     double* logpdf_or_null /* count */);

/* log N(x_s; 0, covscale_s * cov) for S vectors and one dense n x n covariance: the :U => u => :U nodes
 * (generateUfromSigmaU, src/model_likelihood.jl:4-10 with uCov = SigmaU * uNoise; generateU,
 * src/model_prior.jl:27-30).  A non-NULL cov is handed over and cached in the ctx (SigmaU is constant for a data
 * set).  n <= 640: the matrix itself is kept whichever path the call takes (calls the single-workgroup kernels cover scale
 * and factorise it inside one workgroup each; larger calls use its tiled factor, built from the kept matrix when missing or
 * older); n > 640: its tiled factor only.  cov = NULL means the last covariance handed over (here or to gpslc_mvn_draw), for
 * any S; before any hand-over it is an argument error.  S = 0 with a non-NULL cov just hands over and validates (returns the
 * failing pivot if cov is not positive definite).  covscale may be NULL (= 1).  SigmaU is positive definite only by
 * its 1e-13 jitter (src/utils.jl:17-33): every factorisation and solve here is substitution-based (no products with
 * inverted blocks), i.e. backward stable like LAPACK's potrf / trsm. */
int gpslc_mvn_logpdf(gpslc_ctx* ctx, int64_t S, const double* cov, const double* covscale /* S */,
                     const double* x /* n x S */, double* logpdf /* S */);

/* draws[:, s] = chol(covscale_s * cov) z[:, s] for the host's standard normals z: Gen's `mvnormal(zeros(n), uCov)` inside
 * `elliptical_slice(trace, :U => k => :U, zeros(n), uCov)` (uCov = SigmaU * uNoise, src/inference.jl:48-54, 92-98, 233-239,
 * 293-299) and the prior draw of generateUfromSigmaU (src/model_likelihood.jl:4-10).  cov as for gpslc_mvn_logpdf: non-NULL =
 * handed over and cached, NULL = the last covariance handed over to either entry point, for any S; chol(s C) =
 * sqrt(s) chol(C), so one factor serves every uNoise.  n <= 640: the node kernels' draw mode; beyond: the cached tiled
 * factor streamed once per vector by the predictive-draw kernel.  Returns 0, the failing pivot of cov, or a negative status. */
int gpslc_mvn_draw(gpslc_ctx* ctx, int64_t S, const double* cov, const double* covscale /* S */,
                   const double* z /* n x S */, double* draws /* n x S */);

/* ---- src/estimation.jl, src/driver.jl, src/prediction.jl ------------------------------ */

/* The ensemble driver: everything sampleITE / sampleSATE / predictCounterfactualEffects
 * (src/driver.jl:86-89, 108-111; src/prediction.jl:23-36) compute for S posterior samples
 * (the rows extractParameters, src/utils.jl:92-124, would return for nBurnIn:stepSize:nOuter)
 * and L intervention levels doT[0..L).
 *
 *   U       n x nU x S      uyLS  nU x S      xyLS  nX x S      tyLS, yScale, yNoise  S
 *   pred_noise  = hyperparams.predictionCovarianceNoise (src/estimation.jl:82)
 *
 * Outputs (any may be NULL):
 *   meanSATE, varSATE   S x L   (sample index fastest)   conditionalSATE, src/estimation.jl:116-121,
 *                               of Symmetric(CovITE) + pred_noise*I (src/estimation.jl:82, 127-140)
 *   meanITE             n x S x L                         conditionalITE mean, src/estimation.jl:46
 *   ite_draws           L x n x (S*spp), level fastest    predictCounterfactualEffects' `ite`
 *                               (src/prediction.jl:30-33); column order sample-outer/draw-inner
 *                               (src/estimation.jl:100-107)
 * Draws use z_or_null (n x spp x S x L standard normals: z[i + n*(d + spp*(s + S*l))]) when given,
 * else the library's Philox4x32-10 + Box-Muller stream seeded by `seed` (documented in DESIGN.md,
 * restated in oracle/gpslc_oracle.py: stream id = s + S*l, element = i + n*d). */
int gpslc_predict(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                  const double* xyLS, const double* tyLS, const double* yScale,
                  const double* yNoise, int32_t L, const double* doT, double pred_noise,
                  int32_t spp, uint64_t seed, const double* z_or_null,
                  double* meanSATE, double* varSATE, double* meanITE, double* ite_draws);
int gpslc_predict_dev(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                      const double* xyLS, const double* tyLS, const double* yScale,
                      const double* yNoise, int32_t L, const double* doT, double pred_noise,
                      int32_t spp, uint64_t seed, const double* z_or_null,
                      double* meanSATE, double* varSATE, double* meanITE, double* ite_draws);

/* Per-individual interventions (the Vector{Float64} / Vector{Bool} forms of `Intervention`, src/types.jl:138-143): level l
 * is a vector d_l of n values that replaces fill(doT, n) in src/likelihood.jl:27-28 — tyCovLogS = rbfKernelLog(T, d_l, tyLS),
 * tyCovLogSS = rbfKernelLog(d_l, d_l, tyLS) — so CovWWs = B .* G_l, CovWsWs = B .* H_l with G_l[i,j] = exp(-(T_i - d_l[j])^2 /
 * tyLS^2), H_l[i,j] = exp(-(d_l[i] - d_l[j])^2 / tyLS^2).  A Bool vector is passed as 0.0 / 1.0; a scalar doT is exactly the
 * vector fill(doT, n).  (The reference declares these forms for every estimation entry point but fails on them: fill(doT, n)
 * of a vector has no rbfKernelLog method.)  doT is an n x L host array, doT[i + n*l]; every entry must be finite (else
 * -10, "argument #10 is invalid").  Everything else — arguments, outputs and layouts, the normals (z layout, Philox stream
 * s + S*l, gpslc_set_ensemble placement), chunking, schedule and gpslc_last_info — is gpslc_predict's.  Individuals with
 * d_l[i] == T_i get MeanITE exactly 0.0 (row i of CovWWs' - CovWW is identically zero, src/estimation.jl:46); d_l == T gives
 * exact zeros for MeanITE, meanSATE and CovITE - pred_noise*I.  fp64 only: a ctx created with GPSLC_FLAG_FP32_KERNEL returns
 * GPSLC_ERR_UNSUPPORTED.  Each vector level costs passes over the (sample, pair) grid that a scalar level does not
 * (DESIGN.md §11). */
int gpslc_predict_vec(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                      const double* xyLS, const double* tyLS, const double* yScale,
                      const double* yNoise, int32_t L, const double* doT, double pred_noise,
                      int32_t spp, uint64_t seed, const double* z_or_null,
                      double* meanSATE, double* varSATE, double* meanITE, double* ite_draws);

/* Contrasts between two intervention levels: level l is the PAIR (a, b) = (doT[l], doT_base[l]) of scalars and the estimand is
 * "everybody at a" against "everybody at b",
 *     ITE_i(a, b) = f_i(a) - f_i(b)        (gpslc_predict's is f_i(doT) - f_i(T_i): the case "b = the observed treatments"),
 * for a binary treatment with (a, b) = (1, 0) the effect whose average is the ATE E[Y(1) - Y(0)].  With B = yScale exp(Lu + Lx),
 * r^x_j = exp(-(T_j - x)^2 / tyLS^2), rho = exp(-(a - b)^2 / tyLS^2), alpha = (K + yNoise I)^-1 Y:
 *     D = CovWWs_a' - CovWWs_b',  D_ij = B_ij (r^a_j - r^b_j);    MeanITE = D alpha;
 *     CovITE = B ((1 - rho) + (1 - rho)) - D (K + yNoise I)^-1 D',  + pred_noise*I after symmetrisation (src/estimation.jl:82);
 *     meanSATE, varSATE = conditionalSATE of these (src/estimation.jl:116-121).
 * The mean is the difference of two gpslc_predict means; the covariance, varSATE and the draws are NOT obtainable from two
 * gpslc_predict levels (those share the factual term and the whole GP, and draw independently).  doT and doT_base are L host
 * values each, all finite (else -10 / -11, "argument #10 / #11 is invalid").  Everything else — the other arguments, outputs
 * and layouts, NULL conventions, the normals (z layout, Philox stream s + S*l, gpslc_set_ensemble placement), chunking, the
 * schedule and gpslc_last_info — is gpslc_predict's; a contrast level costs what a scalar level costs (no pass over the pairs
 * is added).  Exact identities: a level with a == b gives MeanITE == 0.0 for every individual, meanSATE == 0.0, varSATE ==
 * n*pred_noise/n^2 and CovITE == pred_noise*I, bit for bit.  Accuracy: for |a - b| far below tyLS both r^a - r^b and 1 - rho
 * cancel, so such a pair loses relative accuracy in the mean and, more so, in the variance (1 - rho ~ (a - b)^2 / tyLS^2; the
 * pred_noise jitter then dominates CovITE).  fp64 only: a ctx created with GPSLC_FLAG_FP32_KERNEL returns
 * GPSLC_ERR_UNSUPPORTED.  Not sharded (gpslc_predict_multi keeps gpslc_predict's estimand). */
int gpslc_predict_contrast(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                           const double* xyLS, const double* tyLS, const double* yScale,
                           const double* yNoise, int32_t L, const double* doT, const double* doT_base,
                           double pred_noise, int32_t spp, uint64_t seed, const double* z_or_null,
                           double* meanSATE, double* varSATE, double* meanITE, double* ite_draws);

/* Weighted average effects over groups: tau_w = w' ITE for G weight columns w_g (n values each), the weights used AS GIVEN (no
 * division by n): w = 1/n is the SATE, w = 1_A/|A| the average over a group A (the treated: the ATT; one object of the
 * hierarchy; a stratum), w = 1_A/|A| - 1_B/|B| the difference of two groups with its correct variance (the two group effects
 * are correlated), w = e_i one individual.  For every posterior sample s, level l and column g
 *     meanW = w' MeanITE,    varW = w' (Symmetric(CovITE) + pred_noise*I) w        (src/estimation.jl:46-47, :82)
 * without forming CovITE: with B = yScale exp(Lu + Lx), K = B .* E, bw = B w, kw = K w (one pass over the pairs per sample for all
 * columns and levels), r_j = exp(-(T_j - doT)^2 / tyLS^2):
 *     c = D' w, c_j = r_j bw_j - kw_j;   w' Delta w = sum_j w_j ((kw_j - 2 r_j bw_j) + bw_j);
 *     v = L^-1 c (one more right-hand side of the factorisation of K + yNoise I = L L');
 *     meanW = v . L^-1 Y,   varW = (w' Delta w - v . v) + pred_noise * (w . w).
 * doT_base_or_null == NULL: the estimand of gpslc_predict, f_i(doT) - f_i(T_i).  Otherwise the contrast of gpslc_predict_contrast,
 * f_i(a) - f_i(b) with (a, b) = (doT[l], doT_base[l]): c_j = (r^a_j - r^b_j) bw_j, w' Delta w = ((1 - rho) + (1 - rho)) sum_j w_j bw_j
 * (no kw); a binary treatment, the pair (1, 0) and the mask of the treated give the ATT.
 *   weights   n x G host, weights[i + n*g]; every entry finite (else -13), G >= 1 (else -12)
 *   meanW, varW   S x L x G: element (s, l, g) at s + S*(l + L*g); either may be NULL
 *   meanITE, ite_draws   what gpslc_predict / gpslc_predict_contrast return for the same levels (one call serves both)
 * doT and doT_base are L finite host values each (else -10 / -11); ite_draws with spp < 1 is -15.  Everything else — the other
 * arguments, the normals, chunking, the schedule and gpslc_last_info — is gpslc_predict's.  Exact identities: a zero column gives
 * meanW == 0.0 and varW == 0.0; a level with a == b, or T_i == doT for every i, gives meanW == 0.0 and varW == pred_noise * (w . w).
 * Results do not depend on chunking, streams or the schedule and are identical from run to run.  Scalar levels and fp64 only: a ctx
 * created with GPSLC_FLAG_FP32_KERNEL returns GPSLC_ERR_UNSUPPORTED.  Not sharded (gpslc_predict_multi is unchanged).
 *  */
int gpslc_predict_weighted(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                           const double* xyLS, const double* tyLS, const double* yScale,
                           const double* yNoise, int32_t L, const double* doT, const double* doT_base_or_null,
                           int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed,
                           const double* z_or_null, double* meanW, double* varW, double* meanITE,
                           double* ite_draws);

/* The joint covariance of the weighted effects across the levels of one call: gpslc_predict_weighted with one more output.  A
 * sweep of levels is a dose-response curve; its values tau_l = w_g' ITE_l share one Gaussian process, and simultaneous bands,
 * comparisons of every pair of levels and functionals of the curve (slope, maximum, area) need the L x L covariance of the sweep,
 * which the per-level varW does not give.  With v_l = L^-1 c_l the right-hand sides the weighted call has solved for anyway,
 * bw = B w, kw = K w, beta = w . bw, kappa = w . kw, gamma_l = sum_j w_j r^l_j bw_j and rho(x, y) = exp(-(x - y)^2 / tyLS^2):
 *     Cov(tau_l, tau_l') = P_ll' - v_l . v_l' + [l == l'] pred_noise (w . w)           (the jitter of src/estimation.jl:82 is per level)
 *     ordinary estimand:  P_ll' = rho(d_l, d_l') beta - gamma_l - gamma_l' + kappa
 *     contrast:           P_ll' = [(rho(a_l, a_l') - rho(a_l, b_l')) - (rho(b_l, a_l') - rho(b_l, b_l'))] beta
 * The factorisation is untouched: one Gram pass over the solved rows and O(n L + L^2) prior terms per sample and column.
 *   covW   S x L x L x G host: element (s, l, l', g) at s + S*(l + L*(l' + L*g)); may be NULL (then the call IS
 *          gpslc_predict_weighted: the same kernels are launched)
 * Arguments, layouts, NULL conventions, error codes (-10 / -11 / -12 / -13 / -15, GPSLC_ERR_UNSUPPORTED on a
 * GPSLC_FLAG_FP32_KERNEL ctx), chunking, the schedule and gpslc_last_info are gpslc_predict_weighted's.  Guarantees: every
 * (s, g) block is exactly symmetric (one value is written to both triangles); the diagonal covW[s, l, l, g] is bit-identical
 * to varW[s, l, g] of the same call; meanW, varW, meanITE and ite_draws are bit-identical to gpslc_predict_weighted's with the
 * same arguments; a zero weight column gives an all-0.0 block; a contrast level with a_l == b_l gives row and column l exactly
 * 0.0 off the diagonal; results do not depend on chunking, streams or the factorisation schedule and are identical from run to
 * run.  Near-coincident levels give a block that is semi-definite to rounding (gpslc_curve_samples takes such blocks).
 * Out of scope: cross-covariances between different weight columns (a difference of groups is a weight column), vector levels,
 * the fp32-kernel mode, sharding through gpslc_predict_multi, device-pointer variants.   */
int gpslc_predict_curve(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                        const double* xyLS, const double* tyLS, const double* yScale,
                        const double* yNoise, int32_t L, const double* doT, const double* doT_base_or_null,
                        int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed,
                        const double* z_or_null, double* meanW, double* varW, double* covW, double* meanITE,
                        double* ite_draws);

/* Marginal effects: level l is the slope of individual i's response surface in the treatment at dose a = doT[l], everybody set
 * to that dose,
 *     g_i(a) = d f_i(t) / dt at t = a;
 * its average over the population is the slope of the dose-response curve.  The derivative of a Gaussian process with an RBF
 * kernel is a Gaussian process in closed form: with B = yScale exp(Lu + Lx), wt = 1 / tyLS^2, r^a_j = exp(-(T_j - a)^2 wt),
 * q^a_j = 2 (T_j - a) wt r^a_j (T_j - a formed in fp64), alpha = (K + yNoise I)^-1 Y:
 *     D_ij = Cov(g_i(a), Y_j) = B_ij q^a_j;    MeanITE = D alpha;
 *     CovITE = 2 wt B - D (K + yNoise I)^-1 D',  + pred_noise*I after symmetrisation (src/estimation.jl:82).
 * Nothing cancels (a finite difference of gpslc_predict_contrast loses its mean and, more so, its variance as the two levels
 * approach each other), and a slope level costs what a scalar level costs: only what multiplies B_ij outside the pair loops
 * differs.  doT: L finite host scalars (else -10).
 *   weights_or_null == NULL and G == 0 (the plain form): meanW, varW are S x L with gpslc_predict's meanSATE / varSATE semantics,
 *       the 1/n average: mean = w . z / n, var = (2 wt sum(B) - w . w + n pred_noise) / n^2 with w = L^-1 (q^a .* bsum); covW must be
 *       NULL (else -19)
 *   weights n x G, G >= 1 (the weighted form): meanW, varW S x L x G and covW S x L x L x G (or NULL) with the layouts and
 *       guarantees of gpslc_predict_weighted / gpslc_predict_curve — c_j = q^a_j bw_j, w' Delta w = 2 wt (w . bw) (no kw), and across
 *       the levels P_ll' = (2 wt - 4 (a_l - a_l')^2 wt^2) rho(a_l, a_l') beta; the block is exactly symmetric, its diagonal
 *       bit-identical to varW, a zero weight column gives an all-0.0 block
 *   meanITE n x S x L, ite_draws L x n x (S*spp): the per-individual slope; normals, Philox streams, gpslc_set_ensemble placement,
 *       chunking and gpslc_last_info are gpslc_predict's
 * Errors: G < 0, or G == 0 with weights given: -11; G > 0 with NULL weights, or a non-finite weight: -12; ite_draws with spp < 1:
 * -14; covW without weights: -19.  Scalar levels and fp64 only: a ctx created with GPSLC_FLAG_FP32_KERNEL returns
 * GPSLC_ERR_UNSUPPORTED.  Not sharded (gpslc_predict_multi is unchanged).  A treatment whose values are all equal to a gives a
 * CovITE that is semi-definite to rounding; the draws factorise it robustly, as every CovITE.   */
int gpslc_predict_slope(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                        const double* xyLS, const double* tyLS, const double* yScale,
                        const double* yNoise, int32_t L, const double* doT, int32_t G,
                        const double* weights_or_null, double pred_noise, int32_t spp, uint64_t seed,
                        const double* z_or_null, double* meanW, double* varW, double* covW, double* meanITE,
                        double* ite_draws);

/* Potential outcomes: level l is individual i's expected outcome at dose a = doT[l], everybody set to that dose,
 *     mu_i(a) = f_i(a),
 * the response surface itself and not a difference of it.  Its average over the population is the average dose-response
 * function mu(a) — E[Y(1)] and E[Y(0)] for a binary treatment.  It is the reference's own counterfactual block
 * (src/likelihood.jl:27-49: CovWWs, CovWsWs, CovC22), which conditionalITE only uses inside a difference.  With
 * B = yScale exp(Lu + Lx), wt = 1 / tyLS^2, r^a_j = exp(-(T_j - a)^2 wt), rho(x, y) = exp(-(x - y)^2 wt), alpha = (K + yNoise I)^-1 Y:
 *     D_ij = Cov(f_i(a), Y_j) = B_ij r^a_j;    MeanITE = D alpha   (gpslc_predict's MeanITE without its - (Y_i - yNoise alpha_i),
 *                                                                  and without its exact 0.0 where T_i == a);
 *     CovITE = B - D (K + yNoise I)^-1 D' (= CovC22),  + pred_noise*I after symmetrisation (src/estimation.jl:82).
 * The prior mean is zero as in the reference's model (MvNormal(0, cov)): far from the data mu_i(a) returns to 0, not to the sample
 * mean of Y.  This is the latent surface: the predictive distribution of a new observation adds yNoise_s to the diagonal, which
 * is left to the caller.  An outcome level costs what a scalar level costs: only what multiplies B_ij outside the pair loops
 * differs.  doT: L finite host scalars (else -10).
 *   weights_or_null == NULL and G == 0 (the plain form): meanW, varW are S x L with gpslc_predict's meanSATE / varSATE semantics,
 *       the 1/n average: mean = w . z / n, var = (sum(B) - w . w + n pred_noise) / n^2 with w = L^-1 (r^a .* bsum); covW must be NULL
 *       (else -19)
 *   weights n x G, G >= 1 (the weighted form): meanW, varW S x L x G and covW S x L x L x G (or NULL) with the layouts and
 *       guarantees of gpslc_predict_weighted / gpslc_predict_curve — c_j = r^a_j bw_j, w' Delta w = beta = w . bw (no kw), and across
 *       the levels P_ll' = rho(a_l, a_l') beta; the block is exactly symmetric, its diagonal bit-identical to varW, a zero weight
 *       column gives an all-0.0 block
 *   meanITE n x S x L, ite_draws L x n x (S*spp): the per-individual outcome; normals, Philox streams, gpslc_set_ensemble
 *       placement, chunking and gpslc_last_info are gpslc_predict's
 * Errors: G < 0, or G == 0 with weights given: -11; G > 0 with NULL weights, or a non-finite weight: -12; ite_draws with spp < 1:
 * -14; covW without weights: -19.  fp64 only: a ctx created with GPSLC_FLAG_FP32_KERNEL returns GPSLC_ERR_UNSUPPORTED.  No _dev
 * variant; not sharded (gpslc_predict_multi is unchanged).  Where B is constant (no U and X effect) CovITE is semi-definite to
 * rounding; the draws factorise it robustly, as every CovITE.   */
int gpslc_predict_outcome(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                          const double* xyLS, const double* tyLS, const double* yScale,
                          const double* yNoise, int32_t L, const double* doT, int32_t G,
                          const double* weights_or_null, double pred_noise, int32_t spp, uint64_t seed,
                          const double* z_or_null, double* meanW, double* varW, double* covW, double* meanITE,
                          double* ite_draws);

/* Potential outcomes at per-individual levels: level l sets individual i to d_l[i] = doT[i + n*l] (an n x L host array, every
 * entry finite, else -10), mu_i(d_l[i]) = f_i(d_l[i]).  meanSATE / varSATE are the VALUE OF THE TREATMENT POLICY d_l,
 * V(d_l) = (1/n) sum_i f_i(d_l[i]), and its variance.  With g_ji = rho(T_j, d_i) and h_ij = rho(d_i, d_j):
 *     D_ij = B_ij g_ji,   Delta_ij = B_ij h_ij,   MeanITE_i = sum_j B_ij g_ji alpha_j,   CovITE = Delta - D (K + yNoise I)^-1 D'
 * — gpslc_predict_vec's passes with the factual terms dropped: no K alpha term and no exact 0.0 where d_l[i] == T_i.  d_l == T
 * is the fitted surface: mean K alpha = Y - yNoise alpha and covariance the reference's CovC11; fill(a, n) is the scalar level
 * a of gpslc_predict_outcome.  Signature, layouts, normals, chunking (results are bit-reproducible and independent of it),
 * gpslc_last_info and error codes are gpslc_predict_vec's.  No weights with vector levels.  fp64 only
 * (GPSLC_ERR_UNSUPPORTED on a GPSLC_FLAG_FP32_KERNEL ctx); no _dev variant; not sharded.   */
int gpslc_predict_outcome_vec(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                              const double* xyLS, const double* tyLS, const double* yScale,
                              const double* yNoise, int32_t L, const double* doT, double pred_noise,
                              int32_t spp, uint64_t seed, const double* z_or_null,
                              double* meanSATE, double* varSATE, double* meanITE, double* ite_draws);

/* Predictions for NEW individuals: m individuals that are not in the data, with covariates x*_i (Xnew, m x nX column-major; NULL
 * iff nX == 0) and, per posterior sample, latent confounders u*_i(s) (Unew, m x nU x S; NULL iff nU == 0) — the caller's to
 * supply: a new member of a known object copies a member's U[:, :, s]; an unseen object would need an integral over its U, which
 * is not closed form and not offered.  No reference counterpart: the textbook GP prediction at new inputs from the factorisation
 * of gpslc_predict.  Per sample, with w*_i = [u*_i(s) | x*_i], B*_ij = yScale exp(-sum_f ((w*_if - w_jf) / l_f)^2) (m x n), B** the
 * same between two new individuals, A = K + yNoise I = L L', alpha = A^-1 Y, and for level l of one of the three forms
 *     GPSLC_NEW_OUTCOME   f*(a), a = doT[l]                          cross_j = r^a_j                  prior = 1
 *     GPSLC_NEW_CONTRAST  f*(a) - f*(b), b = doT_base[l] (the CATE)  cross_j = r^a_j - r^b_j          prior = 2 (1 - rho(a, b))
 *     GPSLC_NEW_SLOPE     d f*(t) / dt at t = a                      cross_j = 2 (T_j - a) r^a_j / tyLS^2   prior = 2 / tyLS^2
 * (r^x_j = rho(T_j, x), rho(x, y) = exp(-(x - y)^2 / tyLS^2); the latent surface, no yNoise):
 *     D*_ij = B*_ij cross_j      mean_i = sum_j D*_ij alpha_j      W* = D* L^-T
 *     var_i = (prior yScale - ||row i of W*||^2) + pred_noise      cov_ii' = prior B**_ii' - (W* W*')_ii' + pred_noise [i == i']
 * The ordinary effect f(a) - f(T_i) needs a factual treatment of the new individual: it is the contrast with b = T*, and no form
 * of this call.  doT (L) and doT_base (L; contrast only, else NULL) are finite scalars.
 * Outputs (host; each may be NULL, not all three): mean, var m x S x L — element (i, s, l) at i + m*(s + S*l); cov m x m x S x L —
 * element (i, i', s, l) at i + m*(i' + m*(s + S*l)), exactly symmetric, its diagonal bit-identical to var.  mean and var of a new
 * individual do not depend on which others share the call; every output is bit-reproducible and independent of chunking, streams
 * and the factorisation schedule.  A new individual that copies a training individual (same x, same u(s)) reproduces that
 * individual's row of gpslc_ite_distributions_outcome / _contrast / _slope.  A contrast with a == b gives mean 0.0, var pred_noise
 * and off-diagonal cov 0.0 exactly.  A sample whose factorisation breaks down gets NaN in all its outputs; the call returns the
 * first failing pivot and gpslc_last_info every sample's, as gpslc_y_loo.
 * Errors: m < 1: -9; Xnew / Unew NULL-ness against nX / nU, or a non-finite entry: -10 / -11; unknown form: -12; L < 1: -13; doT
 * NULL or non-finite: -14; doT_base missing for a contrast, given for another form, or non-finite: -15; all outputs NULL: -17.
 * fp64 only (GPSLC_ERR_UNSUPPORTED on a GPSLC_FLAG_FP32_KERNEL ctx); no _dev variant; not sharded; no draws.   */
#define GPSLC_NEW_OUTCOME 0
#define GPSLC_NEW_CONTRAST 1
#define GPSLC_NEW_SLOPE 2
int gpslc_predict_new(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                      const double* tyLS, const double* yScale, const double* yNoise, int64_t m,
                      const double* Xnew, const double* Unew, int32_t form, int32_t L, const double* doT,
                      const double* doT_base, double pred_noise, double* mean, double* var, double* cov);

/* gpslc_predict_new at levels that depend on the new individual: level l sets new individual i to the dose a_il = doT[i + m*l]
 * (m x L host, every entry finite) and, for a contrast, against b_il = doT_base[i + m*l] (m x L; else NULL) — a policy for a new
 * population, or with b_il = T*_i the ordinary effect f*(a) - f*(T*_i) of a new individual whose factual treatment is known.
 * Arguments, output layouts, NULL conventions, NaN and status behaviour are gpslc_predict_new's.  Forms: GPSLC_NEW_OUTCOME and
 * GPSLC_NEW_CONTRAST; GPSLC_NEW_SLOPE is refused (-12, "unsupported form").  Per sample, in the notation above:
 *     cross_ij = rho(T_j, a_il) [- rho(T_j, b_il)]      D*_ij = B*_ij cross_ij      mean_i = sum_j D*_ij alpha_j      W* = D* L^-T
 *     P_ii' = rho(a_i, a_i')   |   (rho(a_i, a_i') - rho(a_i, b_i')) - (rho(b_i, a_i') - rho(b_i, b_i'))
 *     var_i = (P_ii yScale - ||row i of W*||^2) + pred_noise      cov_ii' = P_ii' B**_ii' - (W* W*')_ii' + pred_noise [i == i']
 * cross does not factor into a per-column term: the mean is a pass over the m n pairs per level (one exp per pair and level for the
 * outcome, two for the contrast), not gpslc_predict_new's matrix product.
 * Exact identities: cov is exactly symmetric and its diagonal bit-identical to var; a row with a_il == b_il has mean 0.0, var
 * pred_noise and 0.0 in its row and column of cov off the diagonal; mean and var of a new individual do not depend on which others
 * share the call, and every output is bit-reproducible and independent of chunking, streams and the factorisation schedule.
 * Doses that are the same for every new individual give gpslc_predict_new's results to rounding (var and cov from the same
 * tiles, the mean in another summation order).
 * Errors: gpslc_predict_new's (-9 ... -17; doT / doT_base are checked over their m x L entries); GPSLC_NEW_SLOPE: -12.  fp64 only
 * (GPSLC_ERR_UNSUPPORTED on a GPSLC_FLAG_FP32_KERNEL ctx); no _dev variant; not sharded; no draws.   */
int gpslc_predict_new_vec(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                          const double* tyLS, const double* yScale, const double* yNoise, int64_t m,
                          const double* Xnew, const double* Unew, int32_t form, int32_t L, const double* doT,
                          const double* doT_base, double pred_noise, double* mean, double* var, double* cov);

/* The score of a held-out test set: m individuals the chain has never seen, with covariates Xtest (m x nX; NULL iff nX == 0),
 * latent confounders Utest (m x nU x S; NULL iff nU == 0: gpslc_predict_new's Unew), treatments Ttest (m) and outcomes Ytest (m),
 * every entry finite.  Per posterior sample this is gpslc_predict_new_vec's outcome form with L = 1, a_i = Ttest_i and the
 * OBSERVATION's noise: yNoise_s takes the place of pred_noise in var and on the diagonal of C = B** o P - W* W*' + yNoise I.
 *   mean[i + m*s], var[i + m*s]     the predictive mean and variance of Ytest_i given the n training individuals
 *   lpd[i + m*s]                    log N(Ytest_i; mean, var): the pointwise log predictive density
 *   lpd_joint[s]                    log N(Ytest; mean, C) = -(m/2) log(2 pi) - log det(C)/2 - r' C^-1 r / 2, r = Ytest - mean
 * C is built as 128 x 128 tiles (mt = ceil(m / 128) tile rows) with r as its augmented row and factorised by the kernels that
 * factorise A (gpslc_y_kfold's recipe); log det and the quadratic form come from that factor.  By the chain rule lpd_joint equals
 * gpslc_y_logpdf of the n + m pooled individuals minus gpslc_y_logpdf of the n training individuals, to rounding; at m = 1 it
 * equals lpd.  Each output may be NULL, not all four.
 * A sample whose factorisation of A breaks down gets NaN in all its outputs; return value (first failing pivot) and
 * gpslc_last_info as gpslc_predict_new.  A sample whose C loses positive definiteness gets NaN in lpd_joint and keeps mean, var and
 * lpd; the return value and gpslc_last_info do not change.  Outputs are bit-reproducible and independent of chunking, streams and
 * the factorisation schedule; mean, var and lpd of a test individual do not depend on the others.
 * Errors: m < 1: -9; Xtest / Utest NULL-ness or a non-finite entry: -10 / -11; Ttest NULL or non-finite: -12; Ytest NULL or
 * non-finite: -13; all outputs NULL: -14.  fp64 only (GPSLC_ERR_UNSUPPORTED on a GPSLC_FLAG_FP32_KERNEL ctx); no _dev variant;
 * not sharded.  S = 0 is an empty call.   */
int gpslc_y_test(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                 const double* tyLS, const double* yScale, const double* yNoise, int64_t m,
                 const double* Xtest, const double* Utest, const double* Ttest, const double* Ytest,
                 double* mean, double* var, double* lpd, double* lpd_joint);

/* Weighted averages over NEW individuals: tau_g(l) = w_g' f*(l) for G weight columns over the m new individuals of
 * gpslc_predict_new — the average effect in a target population that is not the sample (next year's cohort, another hospital, a
 * re-weighted grid of profiles, a held-out fold), its subgroups and their differences — with the variance that var of
 * gpslc_predict_new cannot give (the new individuals share one Gaussian process), and the joint covariance of the L levels.
 * Arguments 2 - 15 are gpslc_predict_new's.  weights: m x G host, weights[i + m*g], every entry finite, used AS GIVEN (1/m: the
 * population average; 1_A / |A|: a subgroup; a difference of two such columns: the difference of two groups with its correct
 * variance; e_i: individual i).  Per sample, in the notation above and with joint_ll' of gpslc_predict_curve's forms:
 *     bw*_g = B*' w_g (n)      beta_g = w_g' B** w_g      c_g(l) = cross(l) .* bw*_g      v_g(l) = L^-1 c_g(l)      z = L^-1 Y
 *     meanW = v_g(l) . z      varW = (prior_l beta_g - v_g(l) . v_g(l)) + pred_noise (w_g . w_g)
 *     covW(l, l') = joint_ll' beta_g - v_g(l) . v_g(l')   (l != l'; the diagonal is varW, copied)
 * — w_g' mean and w_g' cov w_g of gpslc_predict_new, without its m x n tile workspace and without anything m x m: one pass over the
 * m n pairs, one over the m^2 pairs and L G more right-hand sides of the factorisation that runs anyway.
 * Outputs (host; each may be NULL, not all three): meanW, varW S x L x G — element (s, l, g) at s + S*(l + L*g); covW S x L x L x G —
 * element (s, l, l', g) at s + S*(l + L*(l' + L*g)): the layouts of gpslc_predict_weighted / gpslc_predict_curve, so
 * gpslc_curve_samples draws whole curves of the target population.  covW without varW: the device computes varW all the same.
 * Exact identities: a zero column gives meanW == 0.0, varW == 0.0 and an all-0.0 covW block; a contrast with a == b gives meanW
 * == 0.0, varW = pred_noise (w . w) and row and column l of covW 0.0 off the diagonal; every covW block is exactly symmetric and its
 * diagonal bit-identical to varW.  A column's results do not depend on the other columns of the call — to the bits among calls
 * of at most 127 right-hand sides (L G <= 127, one augmented tile row); a larger call takes z . v and v . v from the Schur tiles
 * like every weighted call, and agrees with a smaller one in all but the last bits.  Every output is bit-reproducible and
 * independent of chunking, streams and the factorisation schedule.  A sample whose factorisation breaks down
 * gets NaN in all its outputs; the call returns the first failing pivot and gpslc_last_info every sample's.
 * Errors: -9 ... -15 as gpslc_predict_new; G < 1: -16; weights NULL or non-finite: -17; pred_noise non-finite: -18; all outputs
 * NULL: -19.  fp64 only (GPSLC_ERR_UNSUPPORTED on a GPSLC_FLAG_FP32_KERNEL ctx).  Not offered: a _dev variant, sharding, draws per
 * individual, cross-covariances between weight columns (a difference of groups is a weight column), individuals of unseen
 * objects.   */
int gpslc_predict_new_weighted(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                               const double* tyLS, const double* yScale, const double* yNoise, int64_t m,
                               const double* Xnew, const double* Unew, int32_t form, int32_t L, const double* doT,
                               const double* doT_base, int32_t G, const double* weights, double pred_noise,
                               double* meanW, double* varW, double* covW);

/* The same call sharded over several GPUs of one node: what the loop of predictCounterfactualEffects (src/prediction.jl:30-33)
 * over the posterior samples (src/estimation.jl:78-84) becomes when the ensemble is partitioned.  ctxs[0..nctx) are
 * DISTINCT contexts created with the same (n, nX, nU), one per device (gpslc_create(&ctx_k, device_k, ...)), each holding the data
 * (gpslc_set_data on every one: X, T, Y are replicated, N (D + 2) doubles).  Context k computes the contiguous block
 * [k q + min(k, r), ...) of q = S / nctx (+ 1 for k < r = S mod nctx) posterior samples on its own host thread and its own device;
 * nothing moves between the devices while they compute, and every device copies its block of each result straight into the
 * caller's HOST arrays (the same arrays, layouts and NULL conventions as gpslc_predict).  The library's normals are placed with
 * gpslc_set_ensemble semantics, so seeded draws — like every other output — are bit-identical to ONE gpslc_predict call over all S
 * samples, whatever nctx (several contexts on one device are allowed: that is how the single-GPU tests check it).  A placement set on
 * ctxs[0] beforehand is honoured as the placement of the whole call (one node's share of a larger ensemble).
 * info_or_null (S): the 1-based failing pivot of every sample as gpslc_last_info reports it.  Returns the first negative status of
 * any shard, else the first failing pivot in sample order, else 0; gpslc_last_error(ctxs[0]) names the shard.  Host pointers only. */
int gpslc_predict_multi(int32_t nctx, gpslc_ctx* const* ctxs, int64_t S, const double* U, const double* uyLS,
                        const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                        int32_t L, const double* doT, double pred_noise, int32_t spp, uint64_t seed,
                        const double* z_or_null, double* meanSATE, double* varSATE, double* meanITE,
                        double* ite_draws, int32_t* info_or_null);

/* The partition gpslc_predict_multi uses, for callers who drive the contexts themselves (results LEFT on their devices:
 * gpslc_predict_dev per context after gpslc_set_ensemble(ctx_k, s0, S)): block k of nblocks is the posterior samples [*s0, *s1),
 * sizes differ by at most one, the first S mod nblocks blocks are the longer ones.  Host-only arithmetic (no ctx, no GPU); the
 * same partition as causalgpslc.jl_amd/sharded.py: shard_range. */
int gpslc_shard_range(int64_t S, int32_t nblocks, int32_t k, int64_t* s0, int64_t* s1);

/* ITEDistributions(g, doT) (src/estimation.jl:66-86) for one intervention level, with the
 * reference's output layout: MeanITEs S x n and CovITEs S x n x n, sample index fastest;
 * CovITEs carries the + pred_noise*I of src/estimation.jl:82.  Either output may be NULL. */
int gpslc_ite_distributions(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                            const double* xyLS, const double* tyLS, const double* yScale,
                            const double* yNoise, double doT, double pred_noise,
                            double* MeanITEs, double* CovITEs);

/* ITEDistributions(g, doT) for a per-individual intervention doT (n values, host; see gpslc_predict_vec): same outputs and
 * layouts as gpslc_ite_distributions.  A non-finite entry of doT returns -9.  GPSLC_FLAG_FP32_KERNEL: GPSLC_ERR_UNSUPPORTED. */
int gpslc_ite_distributions_vec(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                                const double* xyLS, const double* tyLS, const double* yScale,
                                const double* yNoise, const double* doT, double pred_noise,
                                double* MeanITEs, double* CovITEs);

/* ITEDistributions for the contrast of the scalar levels doT against doT_base (see gpslc_predict_contrast): same outputs and
 * layouts as gpslc_ite_distributions, CovITEs with its + pred_noise*I.  A non-finite doT returns -9, a non-finite doT_base -10.
 * doT == doT_base: MeanITEs all 0.0 and CovITEs == pred_noise*I exactly.  GPSLC_FLAG_FP32_KERNEL: GPSLC_ERR_UNSUPPORTED. */
int gpslc_ite_distributions_contrast(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                                     const double* xyLS, const double* tyLS, const double* yScale,
                                     const double* yNoise, double doT, double doT_base, double pred_noise,
                                     double* MeanITEs, double* CovITEs);

/* ITEDistributions for the slope d f_i(t) / dt at the scalar level t = doT (see gpslc_predict_slope): same outputs and layouts as
 * gpslc_ite_distributions, CovITEs with its + pred_noise*I.  A non-finite doT returns -9.  GPSLC_FLAG_FP32_KERNEL:
 * GPSLC_ERR_UNSUPPORTED. */
int gpslc_ite_distributions_slope(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                                  const double* xyLS, const double* tyLS, const double* yScale,
                                  const double* yNoise, double doT, double pred_noise,
                                  double* MeanITEs, double* CovITEs);

/* ITEDistributions for the potential outcome f_i(doT) at the scalar level doT (see gpslc_predict_outcome): same outputs and
 * layouts as gpslc_ite_distributions — MeanITEs the outcome means, CovITEs = CovC22 with its + pred_noise*I.  A non-finite doT
 * returns -9.  GPSLC_FLAG_FP32_KERNEL: GPSLC_ERR_UNSUPPORTED. */
int gpslc_ite_distributions_outcome(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                                    const double* xyLS, const double* tyLS, const double* yScale,
                                    const double* yNoise, double doT, double pred_noise,
                                    double* MeanITEs, double* CovITEs);

/* The same for a per-individual level doT (n values, host; see gpslc_predict_outcome_vec): outputs, layouts and error codes are
 * gpslc_ite_distributions_vec's (a non-finite entry returns -9; GPSLC_FLAG_FP32_KERNEL: GPSLC_ERR_UNSUPPORTED). */
int gpslc_ite_distributions_outcome_vec(gpslc_ctx* ctx, int64_t S, const double* U, const double* uyLS,
                                        const double* xyLS, const double* tyLS, const double* yScale,
                                        const double* yNoise, const double* doT, double pred_noise,
                                        double* MeanITEs, double* CovITEs);

/* likelihoodDistribution(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, doT) (src/likelihood.jl:8-52 and
 * its three reduced methods :55-94, :97-136, :139-174) for ONE parameter set, as the reference exports it:
 * the dense n x n blocks CovWW, CovWWs, CovWWp and the four posterior blocks CovC11..CovC22 (:46-49),
 * column-major; any output may be NULL.  (Y, the first element of the reference's tuple, is the caller's.) */
int gpslc_likelihood_distribution(gpslc_ctx* ctx, const double* U, const double* uyLS, const double* xyLS,
                                  double tyLS, double yScale, double yNoise, double doT, double* CovWW,
                                  double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                  double* CovC21, double* CovC22);
/* The same blocks for a per-individual intervention doT (n values, host; see gpslc_predict_vec): CovWWs = B .* G,
 * CovWsWs = B .* H behind CovC12, CovC21, CovC22 (src/likelihood.jl:27-28, 35-39, 46-49).  A non-finite entry of doT returns
 * -8.  Like gpslc_likelihood_distribution this entry point always evaluates in fp64, on any ctx. */
int gpslc_likelihood_distribution_vec(gpslc_ctx* ctx, const double* U, const double* uyLS, const double* xyLS,
                                      double tyLS, double yScale, double yNoise, const double* doT, double* CovWW,
                                      double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                      double* CovC21, double* CovC22);

/* SATEsamples (src/estimation.jl:148-163): out[j*spp + d] = mean[j] + var[j] * z — the variance
 * is used as the standard deviation, as the reference does (src/estimation.jl:159).  Host-only
 * arithmetic; z_or_null (S*spp) or Philox stream `seed`, stream id 2^40 + j. */
int gpslc_sate_samples(const double* meanSATE, const double* varSATE, int64_t S, int32_t spp,
                       uint64_t seed, const double* z_or_null, double* out /* S*spp */);

/* Joint draws of a curve from gpslc_predict_curve's outputs (meanW S x L x G, covW S x L x L x G; the lower triangle of each
 * block is read): out[l + L*(d + spp*(s + S*g))] = meanW[s, l, g] + (F z)_l, F F' = the (s, g) block.  F is the factor of a
 * diagonally pivoted Cholesky mapped back to level order; the factorisation stops at the first pivot <= L * eps * max diag and
 * leaves the remaining columns of F zero, so a semi-definite or slightly indefinite block (near-coincident levels on a smooth
 * curve, repeated levels) is a normal input, not an error.  z_or_null: L x spp x S x G standard normals, z[k + L*(d + spp*(s +
 * S*g))] multiplying column k of F (pivot order), or the library's Philox stream `seed`: stream id 2^41 + s + S*g, element
 * k + L*d.  Host-only arithmetic (no ctx, no GPU).  Errors: meanW / covW NULL -1 / -2, S < 0 -3, L < 1 -4, G < 1 -5, spp < 0 -6,
 * out NULL -9. */
int gpslc_curve_samples(const double* meanW, const double* covW, int64_t S, int32_t L, int32_t G,
                        int32_t spp, uint64_t seed, const double* z_or_null, double* out /* L*spp*S*G */);

/* summarizeEstimates(samples; credible_interval) (src/driver.jl:129-149): per-individual Mean and the
 * (1-ci)/2 and 1-(1-ci)/2 quantiles (Julia's Statistics.quantile, type 7) of an n x m sample matrix
 * (column-major, samples[i + n*j]); rows of up to 16384 samples are sorted in LDS, longer ones (S * spp of a large
 * posterior) go through an exact radix select.  The _dev variant reads device memory with explicit strides
 * (sample (i, j) at samples[i*row_stride + j*col_stride]) so that level l of gpslc_predict_dev's ite_draws
 * (L x n x M, level fastest) is summarised in place with samples = draws + l, row_stride = L,
 * col_stride = L*n, and writes device outputs: the draw tensor never leaves HBM.  Both strides count doubles and must be
 * at least 1: row_stride < 1 returns -5, col_stride < 1 returns -6.  n and m are at most 2^31 - 1 (else -3 / -4), for both
 * entry points. */
int gpslc_summarize(gpslc_ctx* ctx, const double* samples, int64_t n, int64_t m, double credible_interval,
                    double* mean, double* lower, double* upper);
int gpslc_summarize_dev(gpslc_ctx* ctx, const double* samples, int64_t n, int64_t m, int64_t row_stride,
                        int64_t col_stride, double credible_interval, double* mean, double* lower, double* upper);

/* 1-based failing pivot (0 = ok) of every posterior sample of the last predict / y_logpdf /
 * ite_distributions call.  Codes <= n refer to the factorisation of the sample's A = K + yNoise I; codes > n to a CovITE
 * factorisation of the draws (pivot = code - n), that of the sample's lowest-index failing level (the order of the
 * reference's level loop, src/prediction.jl:30-33) — the same code whatever the chunking, streams or repeat.  A failing A
 * takes precedence over the sample's CovITE codes. */
int gpslc_last_info(const gpslc_ctx* ctx, int32_t* info, int64_t S);

/* ---- posterior pack (replaces Serialization of a GPSLCObject, src/io.jl:14-34) ----
 * Flat little-endian file: magic "GPSLCPK1"; 6 x int64 {n, nX, nU, S, binaryT, 0}; 7 x f64 hyper-parameters
 * {nU or -1, nOuter, nMHInner, nESInner, nBurnIn, stepSize, predictionCovarianceNoise} (src/types.jl:22-30);
 * then the f64 arrays X[n,nX] T[n] Y[n] U[n,nU,S] uyLS[nU,S] xyLS[nX,S] tyLS[S] yNoise[S] yScale[S], column-
 * major — what extractParameters (src/utils.jl:92-124) yields for the retained samples, stacked.
 * Host-only functions (no ctx, no GPU). */
typedef struct gpslc_pack_header {
    int64_t n, nX, nU, S, binary_t, reserved;
    double hyper[7];
} gpslc_pack_header;

int gpslc_pack_save(const char* path, const gpslc_pack_header* h, const double* X, const double* T,
                    const double* Y, const double* U, const double* uyLS, const double* xyLS,
                    const double* tyLS, const double* yNoise, const double* yScale);
int gpslc_pack_read_header(const char* path, gpslc_pack_header* h);
/* Reads the data and the posterior samples [s0, s1) (0 <= s0 <= s1 <= S) into caller buffers sized for
 * s1 - s0 samples — a rank of a sharded prediction loads only its own block.  Any output may be NULL (skipped). */
int gpslc_pack_load(const char* path, int64_t s0, int64_t s1, double* X, double* T, double* Y, double* U,
                    double* uyLS, double* xyLS, double* tyLS, double* yNoise, double* yScale);

/* ---- measurement hooks (bench.py, profiles/) ----------------------------------------- */

/* Accumulated HIP-event statistics since the last reset, recorded (on the launching stream) when the ctx was
 * created with GPSLC_FLAG_PROFILE: launches, total device milliseconds, total algorithmic work.  Kernel classes:
 *   0  tile_gemm_nt_kernel<0> in the factorisation of A (trailing updates: the dominant kernel)   work = flop
 *   1  tile_fused_strip_kernel in the factorisation of A (in-panel column update + panel solve)        work = flop
 *   2  the predictive-draw kernels of a launch_draws call (normal generation + triangular product)      work = draws
 *   3  every f64-MFMA tile-update launch of the full-ITE-covariance path (W solve, SYRK, factor)        work = flop
 *   4  potrf_tasks_kernel: the whole factorisation of A as one persistent launch (gpslc_set_task_schedule)
 *      work = flop, textbook count n^3 / 3 + (right-hand sides) n^2 per matrix
 * gpslc_profile_get is class 0. */
int gpslc_profile_reset(gpslc_ctx* ctx);
int gpslc_profile_get(gpslc_ctx* ctx, int64_t* launches, double* total_ms, double* total_flop);
int gpslc_profile_get_class(gpslc_ctx* ctx, int32_t kernel_class, int64_t* launches, double* total_ms,
                            double* total_flop);

/* library / build identification, e.g. "gpslc_hip 0.1 gfx950" */
const char* gpslc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GPSLC_HIP_H */
