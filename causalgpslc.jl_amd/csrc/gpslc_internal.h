// Internal declarations shared by the HIP translation units of libgpslc_hip.so.
// gfx950 (MI355X / CDNA4) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "level_form.h"

// ---------------------------------------------------------------------------------------
// Tiled storage.  Every dense matrix the factorisation touches lives in HBM as 128 x 128
// fp64 tiles (128 KiB, column-major inside the tile: element (r, c) at c*128 + r), so a
// K-slab of a tile is one contiguous run and every global access is a full-line stream.
// A "tile matrix" is addressed through a TRef: lower-packed (tile (i, j), j <= i, at
// i(i+1)/2 + j) or rectangular (i*ld + j).
// ---------------------------------------------------------------------------------------
#define GP_TS 128
#define GP_TSQ (GP_TS * GP_TS)

// MFMA accumulators (v_mfma_f64_16x16x4_f64: four doubles per lane) and 16-byte accesses, for every kernel file
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

#define MAXF 32   // max nU + nX of the kernels that hold the features of a tile's rows in LDS (k_gram.hip, k_solve.hip)

// ---------------------------------------------------------------------------------------
// Per-device launch state.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only
// and one process may hold a ctx per GPU, each driven by its own thread: every kernel
// instantiation remembers, per device, whether the opt-in was applied.  Lock-free; two threads racing on the
// same device both apply the (idempotent) attribute.
// ---------------------------------------------------------------------------------------
#include <atomic>
#include <cstdlib>
#include <type_traits>
struct DeviceOnce {
    std::atomic<unsigned long long> mask{0};
};
inline void lds_opt_in(DeviceOnce& o, const void* fn, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (o.mask.load(std::memory_order_acquire) & bit) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    o.mask.fetch_or(bit, std::memory_order_release);
}
// compute units of the current device (cached per device)
inline int device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int v = cus[dev & 63].load(std::memory_order_relaxed);
    if (v == 0) {
        v = 256;
        (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        cus[dev & 63].store(v, std::memory_order_relaxed);
    }
    return v;
}
// Measurement switches exist only in the -DGPSLC_DIAG build that tools/ and the profiling scripts use (libgpslc_hip_diag.so):
// the timing-only kernel variants (GPSLC_GEMM_DIAG), the in-kernel stamps (GPSLC_GEMM_DBG, GPSLC_GEMM_DBG_FUSEK, GPSLC_GRAM_DBG,
// GPSLC_TASK_DBG, GPSLC_SMALL_STAMPS) and the hand-off variants of the persistent launch (GPSLC_TASK_FENCE).  They are
// instruments, not schedules: the A/B switches of rounds 1-7 are settled and gone ("Retired switches").  In the
// production library the environment cannot change a result or a schedule: every switch reads as its default.
inline int diag_env(const char* name, int dflt) {
#ifdef GPSLC_DIAG
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

struct TRef {
    double* base;        // first tile of batch element 0
    long long bstride;   // doubles between consecutive batch elements
    int kind;            // 0 = lower packed, 1 = rectangular
    int ro, co;          // tile offsets added to (i, j)
    int ld;              // tiles per tile-row (rectangular)
    int bdiv;            // > 1: batch element b uses matrix b / bdiv (several (sample, level) units share one factor of A)
};

__host__ __device__ inline long long tref_index(const TRef& t, int i, int j) {
    long long ii = (long long)i + t.ro, jj = (long long)j + t.co;
    return t.kind == 0 ? ii * (ii + 1) / 2 + jj : ii * (long long)t.ld + jj;
}
__host__ __device__ inline double* tref_tile(const TRef& t, long long b, int i, int j) {
    if (t.bdiv > 1) b /= t.bdiv;
    return t.base + b * t.bstride + tref_index(t, i, j) * (long long)GP_TSQ;
}

// C(i, j) -= sum_{kk in [k0, k1)} A(i, kk) * B(j, kk)^T over a set of output tiles.  The host fills one in through the builders
// of tile_launch.h only (one per kind of launch: rectangle, tile column, lower triangle, task matrix), which own the invariants
// between the fields: ntiles against shape / mi / mj / order, short_row0 with short_rows, F / fk with fuse, sym == 3, skip_gdiag.
struct GemmArgs {
    TRef A, B, C;
    int shape;        // 0: lower triangle (incl. diagonal) of an mi x mi tile square, 1: mi x mj rectangle
    int i0, j0;       // output tile (i, j) = (i0 + ii, j0 + jj)
    int mi, mj;
    int k0, k1;
    int diag_skip;    // DIAGNOSTIC ONLY (GPSLC_GEMM_DIAG): 1 = skip in-loop global loads, 2 = also LDS writes
    int nbatch;
    int ntiles;       // output tiles per batch element
    int short_row0;   // output tile rows >= short_row0 (augmented right-hand-side rows) carry only
    int short_rows;   // `short_rows` live rows: dead 16-row sub-tiles are skipped (0 = feature off)
    int sym;          // 0 / 2 / 3.  Nonzero: A and B are the same tile matrix and C(t, t) needs only its lower triangle.
                      // 2: launch_tile_gemm skips the full-size diagonal tiles, which launch_syrk_diag (36 of 64 sub-tile
                      // products, 9 per wave) or launch_diag_update_potrf computes instead; 3: as 2, and the
                      // augmented-row tiles (short_row0, j) of those columns ride with the diagonal items too
    int fuse;         // 1 (launches of one tile column, mj == 1; k1 == k0 allowed): each item also applies the panel
    TRef F;           //    product with tile (0, fk) of F = the inverted diagonal blocks (see k_tilegemm.hip)
    int fk;
    int skip_gdiag;   // the (short) augmented diagonal tile (short_row0, short_row0) is not an item of this launch: nobody
                      // reads -R R^T (EpiArgs::from_rows)
    int* info;        // launch_diag_update_potrf: per-batch-element info words and the code base of tile row 0 (launch_diag's)
    int info_base;
    int* queue;       // launch_tile_gemm: 16 zero-initialised ints (per-XCD ticket counters [0..8), exit counters [8..16))
                      // owned by the launching stream; the kernel leaves them zeroed again
    const unsigned short* order;  // optional (ii, jj) pairs: output-tile visiting order (L2-blocked), or null
    unsigned long long* dbg;      // diagnostic builds only: per-workgroup s_memtime stamps, or null
};

// per-posterior-sample inputs of the Gram build (device pointers, already offset to sample 0 of the call)
struct SampleParams {
    const double* U;       // n x nU x S
    const double* uyLS;    // nU x S
    const double* xyLS;    // nX x S
    const double* tyLS;    // S
    const double* yScale;  // S
    const double* yNoise;  // S
    long long u_sstride;   // doubles between the U blocks of consecutive samples (n*nU; 0 = shared)
};

// The samples of a chunk and their feature blocks [U_s | X]: what every kernel that evaluates the RBF kernel starts from.  The
// two members carry address arithmetic and one load only; scaled_feature below is the one place that divides by ls.
struct SampleGrid {
    const double* X;   // n x nX (ctx or override)
    const double* T;   // n
    SampleParams p;
    long long s0;      // first sample of this chunk
    int n, nX, nU, nt;
    __host__ __device__ const double* column(long long s, int f) const {      // feature f of sample s: n values
        return f < nU ? p.U + s * p.u_sstride + (long long)f * n : X + (long long)(f - nU) * n;
    }
    __host__ __device__ double lengthscale(long long s, int f) const {
        return f < nU ? p.uyLS[s * nU + f] : p.xyLS[s * nX + (f - nU)];
    }
};

// Element i of a column (a feature, or T) as the RT arithmetic stages it.  fp32 (GPSLC_FLAG_FP32_KERNEL): minus the column's
// first element, subtracted in fp64 BEFORE the value is scaled and rounded to fp32 — the RBF model sees differences only, and
// rounding x / ls itself would cost eps32 |x| / ls per difference, which grows with the distance of the data from the origin
// (a column of calendar years: 1e-4).  One centre per (sample, column), the same in every kernel: the same B_ij everywhere.
// fp64: the value itself, the code it always was (eps64 |x| / ls is 1e-13 at |x| / ls = 1000).
template <typename RT>
__device__ __forceinline__ double centred_value(const double* col, int i) {
    if constexpr (std::is_same<RT, float>::value) return col[i] - col[0];
    else return col[i];
}

// Feature f of individual g as the pair loops take it: (x - x')^2 / ls^2 = (x / ls - x' / ls)^2, and every kernel that
// evaluates B_ij forms x / ls as x * (1.0 / ls): the same product everywhere, so the same B_ij everywhere.  RT = float:
// (x - x_0) * (1.0 / ls), centred_value above.  Its two callers: stage_scaled_features (into LDS, per workgroup) and
// col_operands_kernel (k_gram.hip: into the chunk's operand array, once per sample).
template <typename RT>
__device__ __forceinline__ double scaled_feature(const SampleGrid& a, long long s, int f, int g) {
    return centred_value<RT>(a.column(s, f), g) * (1.0 / a.lengthscale(s, f));
}

// Features / lengthscale of COUNT consecutive individuals from g0 into LDS, by a workgroup of 256 threads: FS >= F rows of
// COUNT, zeros beyond n and in the rows F .. FS - 1.
template <int COUNT, typename RT>
__device__ __forceinline__ void stage_scaled_features(const SampleGrid& a, long long s, int F, int FS, int g0, RT* dst) {
    for (int idx = threadIdx.x; idx < FS * COUNT; idx += 256) {
        const int f = idx / COUNT, r = idx % COUNT;
        dst[idx] = (RT)((f < F && g0 + r < a.n) ? scaled_feature<RT>(a, s, f, g0 + r) : 0.0);
    }
}

// The operand array of a chunk (fp64): per sample b and individual g < Np = 128 nt one row of FP doubles, FP = F rounded up
// to a multiple of 8, at least 8 (a row starts on a 64-byte boundary): entry f is scaled_feature<double>, zero for g >= n and
// f >= F.  It exists so that a pair loop whose column is the same for every lane of a wave can take the column's features through
// scalar loads (gram_sop_kernel, k_gram.hip; ite_mean_sop_kernel, k_solve.hip) instead of staging them in LDS and reading them
// back once per lane.  DESIGN.md §30.
__host__ __device__ inline int col_operand_width(int F) { return F <= 8 ? 8 : (F + 7) & ~7; }     // F = 0 (no features): 8 zeros
struct ColOperandArgs : SampleGrid {
    double* cop;       // [b][Np][FP]
};
void launch_col_operands(const ColOperandArgs& a, int nbatch, hipStream_t st);

// lower-packed tile index t = ii (ii + 1) / 2 + jj, 0 <= jj <= ii, back to (ii, jj)
__host__ __device__ __forceinline__ void tri_decode(int t, int& ii, int& jj) {
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long long)(r + 1) * (r + 2) / 2 <= t) ++r;
    while ((long long)r * (r + 1) / 2 > t) --r;
    ii = r; jj = t - (int)((unsigned)r * (unsigned)(r + 1) / 2u);     // r (r + 1) leaves 32 bits from t = 2^30 on
}

struct GramArgs : SampleGrid {
    TRef M;            // lower-packed tile matrix of the chunk
    double* part;      // [b][2][nt][Np] partial column sums of B (0) and K (1)
    int with_sums;
    int f32;           // evaluate the RBF kernel in fp32 (GPSLC_FLAG_FP32_KERNEL)
    int binary_t;      // every T is 0 or 1: e_ij is 1 or exp(-1/tyLS^2), no per-pair exp (bit-identical)
    unsigned long long* dbg;   // measurement build only: per-workgroup s_memtime stamps [entry, staged, columns done, end], or null
    const double* cop;         // non-null (gram_uses_operands): the chunk's operand array, already filled: gram_sop_kernel builds the tiles
};
// which calls the scalar-operand Gram kernel serves: fp64 and the exact feature counts up to 12 (two rows' features in registers).
// The fp32 mode, the runtime-F instantiation and F = 20 keep gram_kernel.
inline bool gram_uses_operands(int F, bool f32) { return !f32 && (F == 4 || F == 5 || F == 6 || F == 8 || F == 10 || F == 12); }

// ---------------------------------------------------------------------------------------
// The whole left-looking factorisation of a batch as ONE persistent launch (round 6, k_tilegemm.hip: potrf_tasks_kernel).
// Tasks: diag(k) = update + Cholesky + inverse of diagonal tile k (the body of diag_update_potrf_kernel; k = 0: of
// diag_potrf_inv_la_kernel), strip(i, k) = column update + panel product of tile (i, k) (a work item of tile_fused_strip_kernel).
// The host lays the tasks of a launch out as eight ticket queues (one per XCD: a matrix never leaves its queue, so the
// 7 - k strips of a column share the B panel in one L2) in an order in which every task follows its producers; progress
// words per matrix in global memory carry the dependencies between workgroups (agent-scope release / acquire).
// ---------------------------------------------------------------------------------------
#include "task_list.h"     // descriptor layout + the host-built task order (plain C++: tests/c/task_list_test.cpp exercises it on the CPU)
struct PotrfTaskArgs {
    GemmArgs g;             // task_matrix (tile_launch.h): A = B = C = the tile matrix, F = the inverted diagonal blocks, k0 = 0,
                            // short_row0 = nt, short_rows, sym = 3 with an augmented row riding along, info / info_base, nbatch
    const unsigned* list;   // TASK_LIST_HDR header words, then the descriptors of the eight queues
    int* sync;              // TASK_SYNC_HDR + TASK_SYNC_STRIDE * nbatch ints (ticket heads, progress words), all zeroed before every
                            // launch by the launcher's caller
    int* timeout;           // set by a poll that exceeds its bound; one word per context, outside `sync`, so that no later launch
                            // can wipe it: read and cleared once per call, after every chunk has drained (check_task_timeout)
    int nt;
    double* alpha;          // non-null: the list ends every matrix with its back-substitution, alpha = L^-T z -> alpha[b][nt 128]
    int fence_mode;         // measurement build only (0 = release / acquire as documented)
    unsigned long long* dbg;   // measurement build only: per-task stamps, or null
};
void launch_potrf_tasks(const PotrfTaskArgs& a, long long ntasks, int mt, hipStream_t st);

// launchers (implemented in the k_*.hip files); all asynchronous on `st`
void launch_tile_gemm(const GemmArgs& g, hipStream_t st);
void launch_syrk_diag(const GemmArgs& g, int carry_aug, hipStream_t st);   // g.mi full-size diagonal tiles from (i0, i0)
void launch_diag_update_potrf(const GemmArgs& g, int carry_aug, hipStream_t st);  // in-panel diagonal tile: update + factor + inverse
void launch_diag(const TRef& M, int k, double* inv, long long inv_bstride, int* info,
                 int info_base, int nbatch, hipStream_t st);
void launch_gram(const GramArgs& g, int nbatch, hipStream_t st);
// substitution-based (backward-stable) diagonal-tile factorisation and panel solve for near-singular matrices (k_robust.hip)
void launch_diag_robust(const TRef& M, int k, int* info, int info_base, int nbatch, hipStream_t st);
void launch_trsm_robust(const TRef& X, const TRef& L, int k, int i0, int count, int nbatch, hipStream_t st);
// info[g] (if still 0) <- the first nonzero of pair_info[g*lc .. g*lc + lc - 1], g < gs (k_robust.hip)
void launch_fold_pair_info(const int* pair_info, int* info, int gs, int lc, hipStream_t st);

// The levels of a prediction call as every kernel that knows about levels receives them; what each form computes from them is
// level_form.h's table.
struct LevelSet {
    const double* doT;    // device: L scalars, or with vec n x L (level l of individual i at doT[i + n*l])
    const double* base;   // LevelForm<form>::paired: level l is the pair (doT[l], base[l]); else null
    int L;
    int form;             // FORM_*
    int vec;              // vector levels (LevelForm<form>::vector_levels)
};

struct RhsArgs {
    const double* T; const double* Y; const double* tyLS;
    long long y_sstride;   // right-hand side 0 of sample s is Y + s*y_sstride (0 = shared)
    long long s0; int n, nt, naug; int with_sums;
    LevelSet lv;           // lv.L: the levels whose sums and rows this launch forms — 0 for vector levels (launch_vec_sums' work)
    const double* part; double* bsum; double* ksum; double* sumdelta;  // bsum/ksum [b][Np], sumdelta [b][L]
    TRef M;
    int live_rows;   // > 0 (single augmented tile row of <= 32 right-hand sides, epilogue sums from the rows of R): only the
                     // first 32 rows of the augmented tiles are written (right-hand sides, then zeros) and the augmented
                     // diagonal tile not at all — every reader of those tiles touches the live 16- / 32-row blocks only
    // G columns of level sums, right-hand side 1 + l + L*g is level l of column g, rows from bw / kw [b][G][Np].  The plain call
    // is G = 1 with bw = bsum, kw = ksum and W null; weighted effects (W non-null) have G weight columns, bw / kw
    // from launch_wsum, sumdelta [b][L*G] and wnorm2 [b][G] = w_g . w_g
    const double* W; int G;   // device, column g fastest: W[g + G*j]
    const double* bw; const double* kw; double* wnorm2;      // kw is read by the factual form only
};
// sums_given: sumdelta (and wnorm2) are already there and neither prepare kernel runs — the weight columns run over other
// individuals than the n of this grid (launch_new_wsum); W stays null, G and bw are a weighted call's
void launch_rhs(const RhsArgs& r, int nbatch, hipStream_t st, bool sums_given = false);

// weighted column sums BW = B W, KW = K W of a chunk (k_wsum.hip): one pass over the pairs per sample for all G columns
struct WsumArgs : SampleGrid {
    int G;
    const double* W;       // device, column g fastest: W[g + G*j]
    double* bw; double* kw;   // [b][G][Np]; kw is not written when with_k == 0 (only the factual form needs K W)
    int with_k;
    int binary_t;          // as GramArgs::binary_t: the e_ij of the K that is factorised
};
void launch_wsum(const WsumArgs& a, int nbatch, hipStream_t st);

struct EpiArgs {
    TRef M; int n, nt, naug, L; long long s0; long long S;
    const double* sumdelta; double pred_noise;
    double* meanSATE; double* varSATE;   // S x L or null
    double* logdet; double* quad;        // S or null
    int from_rows;   // 1 (single augmented tile row): z.z, z.w_l, w_l.w_l are summed from the rows of R themselves — the
                     // augmented diagonal tile is then never updated (factor_panels(..., skip_aug_diag))
    // weighted effects (null / 0 = the plain form): L counts the wL levels x G right-hand sides (row 1 + l + wL*g),
    // meanSATE / varSATE receive mean = z.v and var = (sumdelta - v.v) + pred_noise * wnorm2[b][g] — no division by n
    const double* wnorm2; int wL;
};
void launch_epilogue(const EpiArgs& e, int nbatch, hipStream_t st);

// joint covariance of the weighted effects across the levels of a call (k_curve.hip); runs after the epilogue
struct CurveArgs {
    TRef M; int n, nt, G; long long s0; long long S;
    const double* T; const double* tyLS;
    LevelSet lv;              // scalar levels
    const double* W;          // device, column g fastest: W[g + G*j]
    const double* bw; const double* kw;   // [b][G][Np] (launch_wsum); kw is read by the factual form only
    double* prior;            // [b][G][L + 2]: beta = w . bw, kappa = w . kw, gamma_l = sum_j w_j r^l_j bw_j
    const double* varW;       // S x L x G, as the epilogue stored it: the diagonal
    double* covW;             // S x L x L x G: element (s, l, l', g) at s + S*(l + L*(l' + L*g))
};
// prior_given: prior[b][g][0] = beta is already there (launch_new_wsum; non-factual forms): curve_prior_kernel does not run, and W,
// bw, kw are not read
void launch_curve(const CurveArgs& a, int nbatch, hipStream_t st, bool prior_given = false);

struct BackArgs {
    TRef M; const double* inv; long long inv_bstride; int nt; int naug;
    double* zwork;   // [b][Np] in: z (copied from the augmented row), out: alpha
};
void launch_backsolve(const BackArgs& a, int nbatch, hipStream_t st);

struct IteMeanArgs : SampleGrid {
    long long S;
    LevelSet lv;           // scalar levels; the forms without fp32 kernels run in fp64 whatever f32 says
    const double* alpha;   // [b][Np]
    const double* Y;       // right-hand side alpha solves for: A alpha = Y (sample s at Y + s*y_sstride)
    long long y_sstride;
    const double* yNoise;  // S (= p.yNoise; kept separate so that the generic node paths can pass their own)
    double* meanITE;       // element (i, s, l) at i*si + s*ss + l*sl
    long long si, ss, sl;
    int f32;
    // the scalar-operand kernel (ite_mean_uses_operands): the chunk's operand array [b][Np][FP] (launch_col_operands) and the level
    // vectors R[b][g][LCT], R = cross_g(l) alpha_g for the L <= LCT levels of the call (launch_ite_levels; zero for g >= n, l >= L)
    const double* cop;
    double* R;
};
// which calls the scalar-operand MeanITE kernel serves: fp64, the VALU rungs LCT = 1 and 4, every feature rung but the widest
// (32 features are 64 SGPRs per column: beyond the budget in one piece).  The others keep ite_mean_kernel and its LDS staging.
inline bool ite_mean_uses_operands(int F, int L, bool f32) { return !f32 && L >= 1 && L <= 4 && F <= 20; }
inline int ite_mean_lct(int L) { return L <= 1 ? 1 : 4; }
void launch_ite_levels(const IteMeanArgs& a, int nbatch, hipStream_t st);    // R from alpha: once per sample, after the solve
void launch_ite_mean(const IteMeanArgs& a, int nbatch, hipStream_t st);

// vector levels (per-individual interventions, k_vec.hip): the level sums and MeanITE as passes over the pairs
struct VecArgs : SampleGrid {
    // launch_vec_sums: c_l into row 1 + l of the augmented tiles of M, 1' Delta_l 1 into sumdelta [b][L] (part: [b][L][nt])
    TRef M; double* part; double* sumdelta;
    LevelSet lv;           // d_l[i] at lv.doT[i + n*l].  KEEP IT HERE: first or last in the struct the ordinary mean kernels (LB = 4 | 8) take
                           // 70 | 88 VGPRs, not 56 | 72, and lose one | two waves per SIMD: their argument loads regroup (profiles/level_form.md)
    // launch_vec_mean: alpha [b][Np] solves (K + yNoise I) alpha = Y; element (i, s, l) at meanITE[i*si + s*ss + l*sl]
    const double* alpha; const double* Y; long long y_sstride;
    double* meanITE; long long si, ss, sl;
};
void launch_vec_sums(const VecArgs& a, int nbatch, hipStream_t st);
void launch_vec_mean(const VecArgs& a, int nbatch, hipStream_t st);

// ---------------------------------------------------------------------------------------
// Leave-one-out predictive checks of the outcome model (k_loo.hip): c = diag(A^-1) = the squared row norms of
// W = L^-T from the chunk's tiled factor.  W is upper block-triangular and lives as a PACKED triangle: tile row i keeps its
// nt - i tiles (i, i) .. (i, nt - 1) as one contiguous run in ascending k — the A operand strip_item streams — at the place a
// lower-packed matrix keeps its row nt - 1 - i: tile (i, k) is tile (nt - 1 - i, k - i) of a lower-packed TRef.
// ---------------------------------------------------------------------------------------
__host__ __device__ inline long long loo_w_index(int nt, int i, int k) {
    const long long r = nt - 1 - i;
    return r * (r + 1) / 2 + (k - i);
}
struct LooArgs {
    const double* inv; long long inv_bstride;   // the inverted diagonal tiles of the factor (Chunk::inv)
    double* W; long long w_bstride;             // [b][nt (nt + 1) / 2 tiles], loo_w_index
    int n, nt; long long s0, S;
    double* c;                                  // [b][Np]: diag(A^-1)
    const double* alpha;                        // [b][Np]: A alpha = Y (the vector ite_mean_kernel reads)
    const double* Y; long long y_sstride;       // sample s at Y + s*y_sstride
    const int* info;                            // S: a sample whose factorisation broke down gets NaN
    double* looMean; double* looVar; double* looLpd;   // n x S each (element (i, s) at i + n*s) or null
};
void launch_loo_init(const LooArgs& a, int nbatch, hipStream_t st);       // W(i, i) = inv(L_ii)^T (the other tiles: zeroed by the caller)
// block diagonal d >= 1 of W (k_tilegemm.hip, strip_item): the items (b, i, i + d), i < nt - d = g.ntiles, of
// W(i, k) = -(sum_{kk = i}^{k - 1} W(i, kk) L(k, kk)^T) inv(L_kk)^T.  g: A = C = W as a lower-packed TRef (ro / co are set per
// item), B = the factor, F = the inverted diagonal tiles, nbatch, ntiles, queue
void launch_loo_diagonal(const GemmArgs& g, int nt, int d, hipStream_t st);
void launch_loo_rownorm(const LooArgs& a, int nbatch, hipStream_t st);    // c_r = sum_{k >= i} sum_col W(i, k)[r, col]^2
void launch_loo_finish(const LooArgs& a, int nbatch, hipStream_t st);     // alpha, c, Y -> looMean, looVar, looLpd for the rows < n

// ---------------------------------------------------------------------------------------
// Leave-group-out predictive checks (k_lgo.hip): for a group I of m <= LGO_MAX_GROUP individuals,
// C = [A^-1]_II = W[I, :] W[I, :]^T from the same packed W, then its m x m Cholesky factor in LDS.  One workgroup per
// (group, sample).  Larger groups need a tiled factorisation of C: refused at gpslc_y_lgo's boundary, taken by gpslc_y_kfold (below).
// ---------------------------------------------------------------------------------------
#define LGO_MAX_GROUP GP_TS
struct LgoArgs {
    const double* W; long long w_bstride;       // [b][nt (nt + 1) / 2 tiles], loo_w_index
    int n, nt; long long s0;
    int G, mmax;                                // groups; members of the largest (sizes the launch's LDS)
    const int* members; const int* offsets;     // rows sorted by (group, row); G + 1 offsets into them
    const double* alpha;                        // [b][Np]
    const double* Y; long long y_sstride;
    const int* info;                            // S: a sample whose factorisation broke down gets NaN
    double* lgoMean; double* lgoVar; double* lgoLpd;   // n x S, n x S, G x S (element (g, s) at g + G*s) or null
    const int* gmap; int ngroups;               // null: workgroup x is group x, all G of them (gpslc_y_lgo); else the launch covers
                                                // the ngroups groups gmap[x] (gpslc_y_kfold's groups of at most LGO_MAX_GROUP)
};
void launch_lgo_groups(const LgoArgs& a, int nbatch, hipStream_t st);

// ---------------------------------------------------------------------------------------
// K-fold cross-validation (k_kfold.hip): the groups of more than LGO_MAX_GROUP members.  C = W[I, :] W[I, :]^T is
// built as an mt x mt triangle of tiles with alpha_I as its augmented row, factorised by factor_panels, and read by the
// back-substitution, the epilogue and §18's launches.  The groups of a launch share mt = ceil(m / 128); batch element b is pair
// p0 + b of the class: (sample (p0 + b) / ng of the chunk, group large[(p0 + b) % ng]).
// ---------------------------------------------------------------------------------------
struct KfoldArgs {
    const double* W; long long w_bstride;       // of A: [sample of the chunk][nt (nt + 1) / 2 tiles], loo_w_index
    int n, nt; long long s0;
    int G;                                      // groups of the call (the stride of cvLpd)
    const int* members; const int* offsets;     // as LgoArgs
    const int* large; int ng; long long p0;     // the class's groups, their count, the launch's first pair
    int mt;                                     // tile rows of C
    const double* alpha;                        // [sample of the chunk][Np]
    const double* Y; long long y_sstride;
    const int* info;                            // S: a sample whose factorisation of A broke down gets NaN
    TRef Cm;                                    // lower packed, mt + 1 tile rows: C, and alpha_I in row 0 of tile row mt
    // kfold_finish_kernel: per pair of the launch, [b][mt 128] and [b]
    const double* u; const double* cdiag;       // C^-1 alpha_I (launch_backsolve), diag(C^-1) (launch_loo_rownorm)
    const double* logdet; const double* quad;   // log det C, alpha_I^T C^-1 alpha_I (launch_epilogue)
    const int* pinfo;                           // nonzero: the factorisation of C broke down, the group gets NaN for this sample
    double* cvMean; double* cvVar; double* cvLpd;      // n x S, n x S, G x S or null
};
void launch_kfold_gram(const KfoldArgs& a, int nbatch, hipStream_t st);       // Cm <- C (identity on the padding) and alpha_I
void launch_kfold_finish(const KfoldArgs& a, int nbatch, hipStream_t st);

// ---------------------------------------------------------------------------------------
// Gradient of the outcome log-likelihood (k_grad.hip): with Q = alpha alpha^T - A^-1, K = A - yNoise I and
// P = Q o K, the lengthscale gradients are sums of P_ij D_ijf^2 and the gradient of U_if a row sum of P_ij D_ijf, D_ijf =
// w_if - w_jf over the raw features w = [U | X | T].  A^-1 = W W^T comes tile by tile from the packed W of the leave-one-out
// checks (loo_w_index) and never reaches memory: the pair kernel forms P on the MFMA accumulators and leaves partial sums,
// every work item in its own slot; the finish kernel adds them in ascending tile order.
// ---------------------------------------------------------------------------------------
struct GradArgs : SampleGrid {
    const double* W; long long w_bstride;       // [b][nt (nt + 1) / 2 tiles], loo_w_index
    long long S;
    const double* alpha;                        // [b][Np]: A alpha = Y
    const double* c;                            // [b][Np]: diag(A^-1), or null (neither dyScale nor dyNoise is asked)
    const double* Y; long long y_sstride;       // sample s at Y + s*y_sstride
    const int* info;                            // S: a sample whose factorisation broke down gets NaN
    double* part_ls;                            // [b][nlow][F]: sum of P D_f^2 of lower tile t (off-diagonal tiles doubled); null: no pair pass
    double* part_u;                             // [b][nt][nt][nU][128]: sum over the columns of tile column tj of P D_f, rows of tile row ti
    int* queue;                                 // the stream's ticket counters (GemmArgs::queue)
    // outputs (device, in the layouts of the arguments they differentiate) or null
    double *dU, *duyLS, *dxyLS, *dtyLS, *dyScale, *dyNoise, *dY;
    int no_t;                                   // node mode (gpslc_nodes_logpdf_grad): the features are [U | X] alone,
                                                // T (null on a context without data) and tyLS are never read
    __host__ __device__ int F() const { return nU + nX + (no_t ? 0 : 1); }
    __host__ __device__ const double* raw_column(long long s, int f) const { return f < nU + nX ? column(s, f) : T; }
    __host__ __device__ double ls(long long s, int f) const { return f < nU + nX ? lengthscale(s, f) : p.tyLS[s]; }
};
void launch_grad_pairs(const GradArgs& a, int nbatch, hipStream_t st);    // needs part_ls (and part_u when nU > 0)
void launch_grad_finish(const GradArgs& a, int nbatch, hipStream_t st);

// ---------------------------------------------------------------------------------------
// Predictions for new individuals (k_new.hip): the rows of B* (m x n) and B** (m x m) come from the caller's
// features [Unew_s | Xnew], the columns of B* from the training grid.  NewGrid is a SampleGrid with that second row source;
// stage_scaled_new_features forms x * (1.0 / ls) as stage_scaled_features does, so a new individual that copies a training
// individual gets that individual's row of B bit for bit.  fp64 only.
// ---------------------------------------------------------------------------------------
struct NewGrid : SampleGrid {
    const double* Xnew;     // m x nX, column-major
    const double* Unew;     // m x nU x S, offset to sample 0 of the call like SampleParams::U
    long long un_sstride;   // doubles between the Unew blocks of consecutive samples (m*nU)
    int m, mt;              // new individuals and their row tiles, mt = ceil(m / 128)
    __host__ __device__ const double* new_column(long long s, int f) const {      // feature f of sample s: m values
        return f < nU ? Unew + s * un_sstride + (long long)f * m : Xnew + (long long)(f - nU) * m;
    }
};
template <int COUNT>
__device__ __forceinline__ void stage_scaled_new_features(const NewGrid& a, long long s, int F, int FS, int g0, double* dst) {
    for (int idx = threadIdx.x; idx < FS * COUNT; idx += 256) {
        const int f = idx / COUNT, r = idx % COUNT;
        dst[idx] = (f < F && g0 + r < a.m) ? a.new_column(s, f)[g0 + r] * (1.0 / a.lengthscale(s, f)) : 0.0;
    }
}
struct NewArgs : NewGrid {
    long long S;
    LevelSet lv;            // scalar levels of a non-factual form
    int l0, lc;             // the tile kernels' batch element b = (sample s0 + b / lc, level l0 + b % lc); the mean kernel's b = sample s0 + b
    double pred_noise;
    const double* alpha;    // [sample of the chunk][Np]: A alpha = Y
    TRef W;                 // mt x nt rectangular: D*(l), then W*(l) = D*(l) L^-T
    TRef Cm;                // lower packed mt: prior_l B** + pred_noise I, then the covariance (base null: not asked for)
    double* mean; double* var;   // m x S x L: element (i, s, l) at i + m*(s + S*l)
    double* cov;            // m x m x S x L: element (i, i', s, l) at i + m*(i' + m*(s + S*l))
    // Per-individual levels (lv.vec): lv.doT and lv.base are m x L, new individual i at level l is set to
    // doT[i + m*l] (against base[i + m*l]); outcome and contrast only.  The test-set score (gpslc_y_test) is the outcome form of
    // such a call with L = 1, doT = the test set's own treatments and the observation's noise:
    const double* noise_s;  // non-null: yNoise of the call's samples takes pred_noise's place (S, offset like SampleParams)
    int score;              // Cm has mt + 1 tile rows, the identity on its padded diagonal and Ytest - mean as its augmented row
    const double* Ytest;    // m
    const int* pinfo;       // [b]: nonzero where the factorisation of the pair's C broke down
    const double* ldq;      // [b] log det C, then [nbatch + b] the quadratic form (launch_epilogue)
    double* lpd;            // m x S or null
    double* lpd_joint;      // S or null
};
void launch_new_mean(const NewArgs& a, int nbatch, hipStream_t st);      // mean = (B* R)[i, l], R[j, l] = cross_j(l) alpha_j, all L levels
void launch_new_build(const NewArgs& a, int nbatch, hipStream_t st);     // W <- D*(l) (zero padding), Cm <- prior_l B** + pred_noise I
void launch_new_var(const NewArgs& a, int nbatch, hipStream_t st);       // var = (prior_l yScale - ||row of W||^2) + pred_noise
void launch_new_gather(const NewArgs& a, int nbatch, hipStream_t st);    // Cm -> cov, both triangles; the diagonal is var
void launch_new_mean_vec(const NewArgs& a, int nbatch, hipStream_t st);  // per-individual levels: the mean as a pass over the pairs
void launch_new_score_rhs(const NewArgs& a, int nbatch, hipStream_t st);     // the augmented row of Cm <- Ytest - mean
void launch_new_score_finish(const NewArgs& a, int nbatch, hipStream_t st);  // mean, var, log det C, the quadratic form -> lpd, lpd_joint

// Weighted averages over the new individuals: what launch_rhs, launch_epilogue and launch_curve read of a weighted
// call — bw, sumdelta, wnorm2 and beta — for G weight columns over the m new individuals, from one pass over the m x n pairs and one
// over the m x m pairs.  Everything downstream is the weighted call's (§13, §14) with RhsArgs::sums_given / CurveArgs::prior_given.
struct NewWsumArgs : NewGrid {
    LevelSet lv;            // scalar levels of a non-factual form: prior_l of sumdelta
    int G;
    const double* W;        // device, column g fastest over the new individuals: W[g + G*i]
    double* bw;             // [b][G][Np]: bw*_g = B*^T w_g (rows j >= n: 0.0)
    double* part;           // [b][mt][G]: row block ti's share of beta_g = w_g' B** w_g
    double* sumdelta;       // [b][L*G]: prior_l beta_g at l + L*g
    double* wnorm2;         // [b][G]: w_g . w_g
    double* prior;          // [b][G][L + 2] (CurveArgs::prior): beta_g into slot 0, 0.0 into slot 1; or null
};
void launch_new_wsum(const NewWsumArgs& a, int nbatch, hipStream_t st);

void launch_rbf_log(const double* X1, const double* X2, long long n, int d, const double* ls,
                    int ls_len, double* out, hipStream_t st);
void launch_process_cov(const double* in, long long n, double scale, double noise, double* out,
                        hipStream_t st);

// unit B (full ITE covariance) helpers
struct DtArgs : SampleGrid {
    LevelSet lv;           // batch element b = (sample s0 + b / lc, level l0 + b % lc); with lv.vec g_ij / g_ji / h_ij per pair
    int l0, lc;
    double pred_noise;
    TRef W;    // nt x nt rectangular: receives D (rows = i, cols = j), D_ij = B_ij (r_j - e_ij)
    TRef Cm;   // lower packed nt: receives Delta + pred_noise*I (identity on the padding)
};
void launch_dt_build(const DtArgs& a, int nbatch, hipStream_t st);

struct GatherCovArgs {
    TRef Cm; int n, nt; long long s0, S; double* out; // out: S x n x n, sample fastest
};
void launch_gather_cov(const GatherCovArgs& a, int nbatch, hipStream_t st);

// blocks of 16 draws the streaming draw kernel works on in a pass of nd <= 128 draws: its template parameter NQ
__host__ __device__ inline int draws_nq(int nd) { return nd <= 16 ? 1 : nd <= 32 ? 2 : nd <= 64 ? 4 : 8; }
// doubles of a unit's operand image (DrawArgs::zt) for spp draws per unit: 16 Np per block of 16 draws of its widest pass
inline size_t draws_image_doubles(int spp, long long Np) { return (size_t)16 * draws_nq(spp < 128 ? spp : 128) * Np; }

struct DrawArgs {
    TRef Lc; int n, nt; long long s0, S; int l, L, spp;   // batch element b = (sample s0 + b / lc, level l + b % lc)
    int lc;
    int d0, nd;           // set by launch_draws, one launch pair per pass: the pass's first draw and its count (<= 128).  spp stays
                          // the unit's total: the stride of z, of the Philox element index and of out
    const double* mean;   // meanITE n x S x L
    const double* z;      // caller's normals, n x spp x S x L, or null: the library's Philox normals (philox.h)
    double* zt;           // workspace [nbatch][draws_image_doubles(spp, 128 nt)] — the normals of one pass (caller's or Philox) in the
                          // MFMA operand image the streaming draw kernel reads (draws_zt_index, k_draws.hip), zero-padded
    unsigned long long seed;
    long long rs0, rS;    // Philox stream of batch element b: (rs0 + b / lc) + rS * (l + b % lc) (gpslc_set_ensemble)
    // element (instance i, sample offset sb = b / lc, level offset lb = b % lc, draw d) of this launch goes to
    // out[obase + sb*osb + lb*osl + i*osi + d*osd]: the reference tensor L x n x (S*spp) directly (L == 1), or the
    // level-sweep staging buffer [sample][level][d][i]
    double* out;
    long long obase, osb, osl, osi, osd;
};
void launch_draws(const DrawArgs& a, int nbatch, hipStream_t st);
void launch_draws_scatter(const double* tmp, double* out, long long n, int L, int spp, long long s0, int nbatch,
                          hipStream_t st);

// generic multivariate-normal pieces (U-prior node and friends)
struct DenseLoadArgs { const double* cov; int n, nt; TRef M; };   // column-major n x n -> lower tiles
void launch_dense_load(const DenseLoadArgs& a, hipStream_t st);
struct RowsRhsArgs { const double* x; long long S; int n, nt, naug; TRef M; int row0; int rect; };   // rows q = x[:, q]
void launch_rows_rhs(const RowsRhsArgs& a, hipStream_t st);
struct QuadRowsArgs { TRef M; int n, nt, naug; long long S; double* logdet; double* quad; };
struct RowNormArgs { TRef W; int nt, naug; long long S; double* quad; };   // quad[q] = ||row q of W||^2
void launch_row_norms(const RowNormArgs& a, hipStream_t st);
void launch_quad_rows(const QuadRowsArgs& a, hipStream_t st);

// likelihoodDistribution (src/likelihood.jl:8-174): dense blocks as rectangular tile matrices
struct LdBuildArgs : SampleGrid {
    double doT;
    TRef K, Ks, KsT, Kss;   // nt x nt rectangular each: CovWW, CovWWs, CovWWs', CovWsWs
    const double* doTv;     // non-null: per-individual intervention d (n, device) instead of the scalar doT
};
void launch_ld_build(const LdBuildArgs& a, hipStream_t st);
struct RectGatherArgs { TRef R; int n, nt; double* out; double diag_add; };   // -> column-major n x n
void launch_rect_gather(const RectGatherArgs& a, hipStream_t st);

// single-launch node score for small n (k_small.hip): one workgroup per node, matrix resident in LDS
struct SmallNode {
    const double* Fs;       // n x nF, column-major, ALREADY divided by the lengthscales: Fs[i, f] = F[i, f] * (1 / ls[f])
    const double* target;   // n
    double scale, noise;
    int nF;
    int gofs;               // gradient launch: where this node's results start in the launch's result block (doubles); else 0
    const double* cov;     // non-null: dense n x n covariance in DEVICE memory (lower triangle read); the matrix is
    double covscale;        //   covscale * cov instead of the RBF Gram matrix (the :U => u => :U prior nodes)
};
#define SMALL_INLINE_NODES 4
struct SmallArgs {
    const SmallNode* nodes; // descriptors of the nodes >= SMALL_INLINE_NODES (device-visible memory)
    SmallNode inl[SMALL_INLINE_NODES];   // the first nodes travel in the kernel arguments: no dependent host-memory read
    int n, NB;              // NB = ceil(n / 16) block rows
    double* out;            // [count][4]: logdet, quad, info (1-based failing pivot, 0 = ok), reserved
    double* stamps;         // measurement build only: [count][8] phase timings, else null
    double* scratch;        // mid-size kernel: per-node device scratch (finished block columns + scaled features)
    long long scratch_stride;
    double* draw;           // non-null: [count][n], node i also returns chol(K_i) * target_i (target = standard normals):
                            //   a draw from N(0, K_i) — the auxiliary vector of an elliptical slice, a prior draw
};
size_t small_gp_lds_bytes(int n, int nF);
void launch_small_gp(const SmallArgs& a, int count, int nF_max, hipStream_t st);
// the score and its gradient in the same launch (k_small.hip); the nodes' staging carries the raw features and
// lengthscales behind the target, node i's results land at gout + nodes[i].gofs
size_t small_grad_lds_bytes(int n, int nF);
void launch_small_grad(const SmallArgs& a, double* gout, int count, int nF_max, hipStream_t st);
// left-looking variant for 176 < n <= 640: only the current block column in LDS, finished columns in an L2-resident scratch
size_t mid_gp_scratch_doubles(int n, int nF);
void launch_mid_gp(const SmallArgs& a, int count, int nF_max, hipStream_t st);

// summarizeEstimates (src/driver.jl:129-149): per-row mean and two type-7 quantiles of an n x m sample matrix
struct SummArgs {
    const double* x; long long rs, cs;   // sample (i, j) at x[i*rs + j*cs]
    int n, m, mpad; double lowerQ, upperQ;
    double* mean; double* lower; double* upper;
};
void launch_summarize(const SummArgs& a, hipStream_t st);
