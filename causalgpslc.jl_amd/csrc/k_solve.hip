// O(N^2) kernels around the factor: back-substitution for alpha = A^-1 Y, the MeanITE pass,
// construction of D / Delta for the full ITE covariance, CovITE gather, the likelihood blocks and summarize (the predictive
// draws: k_draws.hip).
#include "gpslc_internal.h"
#include "gp_math.h"
#include "back_block.h"
#include "pair_mfma.h"
#include <stdexcept>

// ---------------------------------------------------------------------------------------
// Back-substitution L^T alpha = z, right-looking over tile rows i = nt-1 .. 0, two launches per row:
// alpha_i = inv(L_ii)^T z_i (one workgroup per matrix), then z_k -= L(i,k)^T alpha_i for every k < i
// (one workgroup per tile; reads L exactly once: HBM-bound).
// ---------------------------------------------------------------------------------------
// alpha_i = inv(L_ii)^T z_i, one workgroup per matrix
__global__ __launch_bounds__(256) void backsolve_alpha_kernel(BackArgs a, int i, double* alpha) {
    __shared__ double zi[GP_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    const int Np = a.nt * GP_TS;
    if (tid < GP_TS) zi[tid] = a.zwork[b * Np + i * GP_TS + tid];
    __syncthreads();
    const double* invt = a.inv + b * a.inv_bstride + (long long)i * GP_TSQ;
    double o32[32];
    tile_tv32(invt, zi, wave, lane, o32);
    if (lane == 0) {
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) alpha[b * Np + i * GP_TS + wave * 32 + cc] = o32[cc];
    }
}
// z_k -= L(i,k)^T alpha_i for k < i, one workgroup per (k, matrix)
__global__ __launch_bounds__(256) void backsolve_update_kernel(BackArgs a, int i, const double* alpha) {
    __shared__ double ai[GP_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x;
    const long long b = blockIdx.y;
    const int Np = a.nt * GP_TS;
    if (tid < GP_TS) ai[tid] = alpha[b * Np + i * GP_TS + tid];
    __syncthreads();
    double o32[32];
    tile_tv32(tref_tile(a.M, b, i, k), ai, wave, lane, o32);
    double* z = a.zwork + b * Np;
    if (lane == 0) {
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) z[k * GP_TS + wave * 32 + cc] -= o32[cc];
    }
}

// copy z = row 0 of the augmented tile row (nt, j) into zwork
__global__ __launch_bounds__(128) void extract_z_kernel(BackArgs a) {
    const int j = blockIdx.x;
    const long long b = blockIdx.y;
    const double* t = tref_tile(a.M, b, a.nt, j);
    a.zwork[b * a.nt * GP_TS + j * GP_TS + threadIdx.x] = t[threadIdx.x * GP_TS + 0];
}

void launch_backsolve(const BackArgs& a, int nbatch, hipStream_t st) {
    // alpha is stored right behind zwork (caller allocates 2 * nbatch * Np doubles)
    double* alpha = a.zwork + (long long)nbatch * a.nt * GP_TS;
    hipLaunchKernelGGL(extract_z_kernel, dim3(a.nt, nbatch), dim3(128), 0, st, a);
    for (int i = a.nt - 1; i >= 0; --i) {
        hipLaunchKernelGGL(backsolve_alpha_kernel, dim3(nbatch), dim3(256), 0, st, a, i, alpha);
        if (i > 0) hipLaunchKernelGGL(backsolve_update_kernel, dim3(i, nbatch), dim3(256), 0, st, a, i, alpha);
    }
}

// ---------------------------------------------------------------------------------------
// MeanITE (src/estimation.jl:46):  MeanITE = (Ks' - K) alpha,  alpha = A^-1 Y,  Ks'_ij = B_ij r_j(l),  K = B .* E.
// Round 3: K alpha needs no second pass over the pairs — A alpha = Y, so  K alpha = Y - yNoise alpha  comes from the solve
// itself, and
//     MeanITE_i(l) = sum_j B_ij (r_j(l) alpha_j)  -  (Y_i - yNoise alpha_i)
// costs ONE exp per pair (B_ij) instead of two (the e_ij of round 1/2: 56 -> 36 fp64-rate instructions per pair).
// Row i of D = Ks' - K is identically zero in the reference's own arithmetic whenever T_i == doT ((T_j - doT)^2 and
// (T_i - T_j)^2 are then the same square, so Ks'_ij == K_ij bit for bit): the reference returns an exact 0.0 for such an
// instance (test/estimation.jl:6-66 is the n = 1 case) and so does this kernel.
// One workgroup per (row block, sample); levels are processed LCT at a time.
// The level forms (FORM is IteMeanArgs::lv.form, level_form.h) differ in what is staged per column block, cross_j(l) alpha_j, and
// in the store: only the factual form has the K alpha term and the T_i == doT rule; a level that is zero by its form (a contrast
// with a == b stages exact zeros: r^a == r^b bit for bit) is stored as 0.0.  The pair loop is the same code.
// ---------------------------------------------------------------------------------------
// cross_g(l) alpha_g of column g at level l: what the pair loop multiplies B_ig with, for both MeanITE kernels below
template <int FORM, typename RT>
__device__ __forceinline__ double ite_level_value(const IteMeanArgs& a, int g, int l, const double* alpha, double wt, const double* etab) {
    using LF = LevelForm<FORM>;
    const RT wtq = (RT)wt;
    // the difference in fp64, then ONE rounding (fp32 mode): its error does not grow with |T|
    const double dt64 = a.T[g] - a.lv.doT[l];
    const RT dt = (RT)dt64, db = LF::paired ? (RT)(a.T[g] - a.lv.base[l]) : (RT)0;
    const double rb = LF::paired ? (double)RbfMath<RT>::exp_neg_t(-((db * db) * wtq), etab) : 0.0;
    return LF::cross(dt64, (double)RbfMath<RT>::exp_neg_t(-((dt * dt) * wtq), etab), rb, wt) * alpha[g];
}

template <int FREG, int LCT, typename RT, int RB, int FORM = FORM_ORDINARY>
__global__ __launch_bounds__(256) void ite_mean_kernel(IteMeanArgs a) {
    using LF = LevelForm<FORM>;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int F = a.nU + a.nX;
    double* etab = sm;                     // [32] 2^(j/32): table-driven exp (gp_math.h)
    double* rl = etab + GP_EXP_TAB_DOUBLES;   // [LCT][128]  r_j(l) * alpha_j of the staged column block
    double* red = rl + LCT * GP_TS;        // [RB][128][LCT]
    RT* fc = reinterpret_cast<RT*>(red + RB * GP_TS * LCT);   // [FREG][128] column features / LS (zero rows beyond F)
    const int tid = threadIdx.x, r = tid & 127, h = tid >> 7;
    const int ib = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int n = a.n, Np = a.nt * GP_TS;

    auto feat_src = [&](int f) { return a.column(s, f); };
    auto feat_il = [&](int f) { return 1.0 / a.lengthscale(s, f); };
    int gi[RB];
    RT af[RB][FREG];   // this thread's rows' features / LS
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        gi[q] = (ib * RB + q) * GP_TS + r;
#pragma unroll
        for (int f = 0; f < FREG; ++f) af[q][f] = (RT)((f < F && gi[q] < n) ? centred_value<RT>(feat_src(f), gi[q]) * feat_il(f) : 0.0);
    }
    const double ys = a.p.yScale[s];
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    gp_exp_tab_stage(etab, tid);
    const double* alpha = a.alpha + b * Np;

    const int L = a.lv.L;
    const double* doT = a.lv.doT;
    for (int l0 = 0; l0 < L; l0 += LCT) {
        const int nl = min(LCT, L - l0);
        double acc[RB][LCT];
#pragma unroll
        for (int q = 0; q < RB; ++q)
#pragma unroll
            for (int ll = 0; ll < LCT; ++ll) acc[q][ll] = 0.0;
        for (int jt = 0; jt < a.nt; ++jt) {
            __syncthreads();
            stage_scaled_features<GP_TS>(a, s, F, FREG, jt * GP_TS, fc);
            for (int idx = tid; idx < LCT * GP_TS; idx += 256) {
                const int ll = idx >> 7, cc = idx & 127;
                const int g = jt * GP_TS + cc;
                double v = 0.0;
                if (ll < nl && g < n) v = ite_level_value<FORM, RT>(a, g, l0 + ll, alpha, wt, etab);
                rl[idx] = v;
            }
            __syncthreads();
#pragma unroll 2
            for (int cq = 0; cq < 64; ++cq) {
                const int c = h * 64 + cq;
                RT cf[FREG];
#pragma unroll
                for (int f = 0; f < FREG; ++f) cf[f] = fc[f * GP_TS + c];
                double rlc[LCT];
#pragma unroll
                for (int ll = 0; ll < LCT; ++ll) rlc[ll] = rl[ll * GP_TS + c];
#pragma unroll
                for (int q = 0; q < RB; ++q) {
                    RT lux = (RT)0;
#pragma unroll
                    for (int f = 0; f < FREG; ++f) {
                        const RT d = af[q][f] - cf[f];
                        lux = fma(d, d, lux);
                    }
                    const double Bv = (double)((RT)ys * RbfMath<RT>::exp_neg_t(-lux, etab));
#pragma unroll
                    for (int ll = 0; ll < LCT; ++ll) acc[q][ll] = fma(Bv, rlc[ll], acc[q][ll]);
                }
            }
        }
        __syncthreads();
        if (h == 1) {
#pragma unroll
            for (int q = 0; q < RB; ++q)
#pragma unroll
                for (int ll = 0; ll < LCT; ++ll) red[(q * GP_TS + r) * LCT + ll] = acc[q][ll];
        }
        __syncthreads();
        if (h == 0) {
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                if (gi[q] >= n) continue;
                if constexpr (!LF::factual) {
#pragma unroll
                    for (int ll = 0; ll < LCT; ++ll)
                        if (ll < nl) {
                            const double v = acc[q][ll] + red[(q * GP_TS + r) * LCT + ll];
                            a.meanITE[(long long)gi[q] * a.si + s * a.ss + (long long)(l0 + ll) * a.sl] =
                                (LF::paired && LF::zero_level(doT[l0 + ll], a.lv.base[l0 + ll])) ? 0.0 : v;
                        }
                    continue;
                }
                // (K alpha)_i = Y_i - yNoise alpha_i: alpha solves (K + yNoise I) alpha = Y
                const double ka = a.Y[s * a.y_sstride + gi[q]] - a.yNoise[s] * alpha[gi[q]];
                const double ti = a.T[gi[q]];
#pragma unroll
                for (int ll = 0; ll < LCT; ++ll)
                    if (ll < nl) {
                        const double v = (acc[q][ll] + red[(q * GP_TS + r) * LCT + ll]) - ka;
                        a.meanITE[(long long)gi[q] * a.si + s * a.ss + (long long)(l0 + ll) * a.sl] =
                            (ti == doT[l0 + ll]) ? 0.0 : v;
                    }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// The same pass with the column's operands in scalar registers (fp64, LCT = 1 | 4, F <= 20: ite_mean_uses_operands).  In
// ite_mean_kernel the column c = h * 64 + cq is the same for every lane of a wave, yet each lane reads the column's FREG
// features and LCT level values from LDS: the LDS array is then as busy as the VALU.  Here they come through wave-uniform
// addresses, which the compiler turns into scalar loads and scalar operands of the v_add_f64 / v_fma_f64 that use them:
//   - the features from the chunk's operand array (launch_col_operands): one row of FP doubles per (sample, individual);
//   - the level values from R[b][g][LCT] = cross_g(l) alpha_g (ite_levels_kernel below), which every row-block workgroup
//     of a sample recomputed for itself in ite_mean_kernel's staging loop.
// No column tile is staged, so the two barriers per column tile are gone and only the exp table stays in LDS (its index is
// per lane).  The arithmetic of a pair and the order of a row's sum are ite_mean_kernel's: h = 0 takes the columns
// jt * 128 + 0..63 and h = 1 the columns 64..127, each ascending over jt, then acc(h = 0) + red(h = 1).
// The body takes its global arrays as __restrict__ parameters: that is what lets the compiler prove that the store of the
// results cannot change an operand, which a scalar load requires.
// ---------------------------------------------------------------------------------------
// R[b][g][LCT] for the g of one row block; one workgroup per (row block, sample)
template <int LCT, int FORM>
__global__ __launch_bounds__(256) void ite_levels_kernel(IteMeanArgs a) {
    __shared__ double etab[GP_EXP_TAB_DOUBLES];
    const int tid = threadIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int Np = a.nt * GP_TS;
    gp_exp_tab_stage(etab, tid);
    __syncthreads();
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    const double* alpha = a.alpha + b * Np;
    for (int idx = tid; idx < LCT * GP_TS; idx += 256) {
        const int ll = idx % LCT, g = blockIdx.x * GP_TS + idx / LCT;
        double v = 0.0;
        if (ll < a.lv.L && g < a.n) v = ite_level_value<FORM, double>(a, g, ll, alpha, wt, etab);
        a.R[(b * Np + g) * LCT + ll] = v;
    }
}

template <int FREG, int LCT, int FORM>
__device__ __forceinline__ void ite_mean_sop_body(const IteMeanArgs& a, const double* __restrict__ cop, const double* __restrict__ R,
                                                  double* __restrict__ out, const double* etab, double* red) {
    using LF = LevelForm<FORM>;
    const int tid = threadIdx.x, r = tid & 127;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 7);     // the same for a whole wave: keeps the column addresses scalar
    const int ib = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int n = a.n, Np = a.nt * GP_TS, L = a.lv.L;
    const int FP = col_operand_width(a.nU + a.nX);
    const int gi = ib * GP_TS + r;

    double af[FREG];   // this thread's row's features / LS: its row of the operand array (zeros beyond n and F)
    {
        const double* rowp = cop + (b * Np + gi) * FP;
#pragma unroll
        for (int f = 0; f < FREG; ++f) af[f] = rowp[f];
    }
    const double ys = a.p.yScale[s];
    double acc[LCT];
#pragma unroll
    for (int ll = 0; ll < LCT; ++ll) acc[ll] = 0.0;
    for (int jt = 0; jt < a.nt; ++jt) {
        const long long c0 = b * Np + jt * GP_TS + h * 64;
        const double* __restrict__ cp = cop + c0 * FP;
        const double* __restrict__ rp = R + c0 * LCT;
#pragma unroll 2
        for (int cq = 0; cq < 64; ++cq) {
            double lux = 0.0;
#pragma unroll
            for (int f = 0; f < FREG; ++f) {
                const double d = af[f] - cp[cq * FP + f];
                lux = fma(d, d, lux);
            }
            const double Bv = ys * gp_exp_neg_tab(-lux, etab);
#pragma unroll
            for (int ll = 0; ll < LCT; ++ll) acc[ll] = fma(Bv, rp[cq * LCT + ll], acc[ll]);
        }
    }
    if (h == 1) {
#pragma unroll
        for (int ll = 0; ll < LCT; ++ll) red[r * LCT + ll] = acc[ll];
    }
    __syncthreads();
    if (h != 0 || gi >= n) return;
    const double* doT = a.lv.doT;
    if constexpr (!LF::factual) {
#pragma unroll
        for (int ll = 0; ll < LCT; ++ll)
            if (ll < L) {
                const double v = acc[ll] + red[r * LCT + ll];
                out[(long long)gi * a.si + s * a.ss + (long long)ll * a.sl] = (LF::paired && LF::zero_level(doT[ll], a.lv.base[ll])) ? 0.0 : v;
            }
    } else {
        // (K alpha)_i = Y_i - yNoise alpha_i: alpha solves (K + yNoise I) alpha = Y
        const double ka = a.Y[s * a.y_sstride + gi] - a.yNoise[s] * a.alpha[b * Np + gi];
        const double ti = a.T[gi];
#pragma unroll
        for (int ll = 0; ll < LCT; ++ll)
            if (ll < L) {
                const double v = (acc[ll] + red[r * LCT + ll]) - ka;
                out[(long long)gi * a.si + s * a.ss + (long long)ll * a.sl] = (ti == doT[ll]) ? 0.0 : v;
            }
    }
}

template <int FREG, int LCT, int FORM>
__global__ __launch_bounds__(256) void ite_mean_sop_kernel(IteMeanArgs a) {
    __shared__ double etab[GP_EXP_TAB_DOUBLES];     // 2^(j/32): table-driven exp (gp_math.h)
    __shared__ double red[GP_TS * LCT];
    gp_exp_tab_stage(etab, threadIdx.x);
    __syncthreads();
    ite_mean_sop_body<FREG, LCT, FORM>(a, a.cop, a.R, a.meanITE, etab, red);
}

// ---------------------------------------------------------------------------------------
// MeanITE for many intervention levels on the MFMA (L > 4, fp64):
//   MeanITE[i, l] = sum_j B_ij (r_j(l) alpha_j)  -  (Y_i - yNoise alpha_i)
// = (B R)[i, l] - (K alpha)[i],  R[j, l] = r_j(l) alpha_j  — a (128 x N)(N x 64) product per row block; K alpha from
// the solve itself (A alpha = Y; see ite_mean_kernel), so the pair loop evaluates one exp (B_ij) and no e_ij.
// The product is the pair-product body this kernel shares with wsum_mfma_kernel (pair_mfma.h: no operand tile of B goes
// through LDS, each lane computes its own B_rc, R is staged per 64-column chunk, fixed summation order, and why the FREG
// rung that serves an F cannot change a bit).  This kernel supplies the two things the body asks of a caller:
//   - what is staged: R[j, l] = cross_j(l) alpha_j of the level form (level_form.h), r_j(l) alpha_j for the ordinary one;
//   - the store, per 16-row sub-tile: rows i < n only, (K alpha)_i and T_i loaded once; instances with T_i == doT_l get the
//     reference's exact 0.0 (row i of Ks' - K is identically zero there).  Without a factual term: no K alpha term, and 0.0
//     only for a level that is zero by its form, as in ite_mean_kernel.
// ---------------------------------------------------------------------------------------
template <int FREG, int FORM = FORM_ORDINARY>   // FREG > 0: this lane's two rows' features live in registers (F <= FREG); 0: read from LDS
__global__ __launch_bounds__(256, 2) void ite_mean_mfma_kernel(IteMeanArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const long long b = blockIdx.y, s = a.s0 + b;
    const double* alpha = a.alpha + b * (a.nt * GP_TS);
    using LF = LevelForm<FORM>;
    const double* doT = a.lv.doT;
    pair_mfma_body<FREG, false, 0>(
        a, s, a.lv.L, sm,
        [&](int j, int l, double wt, const double* etab) {
            const double dt = a.T[j] - doT[l], db = LF::paired ? a.T[j] - a.lv.base[l] : 0.0;
            const double rb = LF::paired ? gp_exp_neg_tab(-((db * db) * wt), etab) : 0.0;
            return LF::cross(dt, gp_exp_neg_tab(-((dt * dt) * wt), etab), rb, wt) * alpha[j];
        },
        [&](int gi, int l0, int nl, const d4* acc, const d4*) {
            if (gi >= a.n) return;
            double* out = a.meanITE + (long long)gi * a.si + s * a.ss;
            if constexpr (!LF::factual) {
                pair_mfma_each_column(nl, [&](int q, int v, int ll) {
                    out[(long long)(l0 + ll) * a.sl] = (LF::paired && LF::zero_level(doT[l0 + ll], a.lv.base[l0 + ll])) ? 0.0 : acc[q][v];
                });
                return;
            }
            const double ka = a.Y[s * a.y_sstride + gi] - a.yNoise[s] * alpha[gi];     // (K alpha)_i from A alpha = Y
            const double ti = a.T[gi];
            pair_mfma_each_column(nl, [&](int q, int v, int ll) {
                out[(long long)(l0 + ll) * a.sl] = (ti == doT[l0 + ll]) ? 0.0 : acc[q][v] - ka;
            });
        });
}

template <int FORM>
static void launch_ite_mean_mfma(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    pair_mfma_freg_ladder(a.nU + a.nX, [&](auto freg) {
        constexpr int FREG = decltype(freg)::value;
        pair_mfma_launch<ite_mean_mfma_kernel<FREG, FORM>, FREG, false>(a, nbatch, st);
    });
}

template <int FREG, int LCT, typename RT, int FORM>
static void launch_ite_mean_t(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    constexpr int RB = 1;     // row blocks per workgroup (2 measured slower: occupancy)
    const int bytes = (GP_EXP_TAB_DOUBLES + (1 + RB) * LCT * GP_TS) * 8 + (FREG * GP_TS) * (int)sizeof(RT);
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)ite_mean_kernel<FREG, LCT, RT, RB, FORM>, bytes);
    hipLaunchKernelGGL((ite_mean_kernel<FREG, LCT, RT, RB, FORM>), dim3((a.nt + RB - 1) / RB, nbatch), dim3(256), bytes, st, a);
}
template <int FREG, typename RT, int FORM>
static void launch_ite_mean_f(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    // a.cop: the caller prepared the operand array and R (ite_mean_uses_operands): the scalar-operand kernel, one workgroup per
    // (row block, sample) as below
    if constexpr (std::is_same<RT, double>::value && FREG <= 20) {
        if (a.cop) {
            if (a.lv.L <= 1) hipLaunchKernelGGL((ite_mean_sop_kernel<FREG, 1, FORM>), dim3(a.nt, nbatch), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((ite_mean_sop_kernel<FREG, 4, FORM>), dim3(a.nt, nbatch), dim3(256), 0, st, a);
            return;
        }
    }
    if (a.lv.L <= 1) launch_ite_mean_t<FREG, 1, RT, FORM>(a, nbatch, st);
    else if (a.lv.L <= 4) launch_ite_mean_t<FREG, 4, RT, FORM>(a, nbatch, st);
    // L > 4 reaches this VALU ladder in the fp32 mode only (fp64: the MFMA kernel, launch_ite_mean), so only the forms with it get the rung
    else if constexpr (LevelForm<FORM>::fp32_kernels) launch_ite_mean_t<FREG, 16, RT, FORM>(a, nbatch, st);
}
template <typename RT, int FORM>
static void launch_ite_mean_r(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    // exact register counts for the common feature widths: the pass is fp64-VALU bound (2 instructions per
    // feature per element), a padded feature is paid in full
    if (F <= 4) launch_ite_mean_f<4, RT, FORM>(a, nbatch, st);
    else if (F <= 5) launch_ite_mean_f<5, RT, FORM>(a, nbatch, st);      // BASELINE config 2: nU + nX = 1 + 4
    else if (F <= 6) launch_ite_mean_f<6, RT, FORM>(a, nbatch, st);
    else if (F <= 8) launch_ite_mean_f<8, RT, FORM>(a, nbatch, st);
    else if (F <= 10) launch_ite_mean_f<10, RT, FORM>(a, nbatch, st);
    else if (F <= 12) launch_ite_mean_f<12, RT, FORM>(a, nbatch, st);
    else if (F <= 16) launch_ite_mean_f<16, RT, FORM>(a, nbatch, st);
    else if (F <= 20) launch_ite_mean_f<20, RT, FORM>(a, nbatch, st);
    else launch_ite_mean_f<32, RT, FORM>(a, nbatch, st);
}
void launch_ite_levels(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    dispatch_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        if (ite_mean_lct(a.lv.L) == 1) hipLaunchKernelGGL((ite_levels_kernel<1, FORM>), dim3(a.nt, nbatch), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ite_levels_kernel<4, FORM>), dim3(a.nt, nbatch), dim3(256), 0, st, a);
    });
}
void launch_ite_mean(const IteMeanArgs& a, int nbatch, hipStream_t st) {
    dispatch_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        // the fp32 mode keeps the VALU kernel for every L; the forms without it (the entry points refuse the mode) run in fp64
        if constexpr (LevelForm<FORM>::fp32_kernels) {
            if (a.f32) { launch_ite_mean_r<float, FORM>(a, nbatch, st); return; }
        }
        // many levels: the (B R) product belongs on the matrix cores
        if (a.lv.L > 4) launch_ite_mean_mfma<FORM>(a, nbatch, st);
        else launch_ite_mean_r<double, FORM>(a, nbatch, st);
    });
}

// ---------------------------------------------------------------------------------------
// The tile builders: one workgroup fills one 128 x 128 tile of every matrix whose element (i, j) is B_ij times a function of the
// treatment kernel's values at the pair — D / Delta of the full ITE covariance (dt_build_kernel) and the four likelihood blocks
// (ld_build_kernel).  tile_build_body is what they share: the LDS layout, the staging, the thread mapping (thread (ty, tx) owns
// rows ty + 16p and columns 8 tx + q, as gram_kernel), (x/l - x'/l)^2 summed by fma in feature order, B_ij = yScale exp(-lux).
// With rho(x, y) = exp(-(x - y)^2 / tyLS^2) (gp_rho) an element's level terms are
//     e = rho(T_i, T_j)      g_ij = rho(T_i, d_j)      g_ji = rho(T_j, d_i)      h = rho(d_i, d_j)
// for a per-individual intervention d (LEVEL_VECTOR; rr_ / rc_ hold d of the row / column block), and a scalar level doT is the
// case g_ij = r_i, g_ji = r_j, h = 1 with r_i = rho(T_i, doT) staged in rr_ / rc_ (LEVEL_SCALAR).  LEVEL_NONE (contrasts) stages
// the column block's values only, hands them over as g_ji and evaluates neither e nor the other terms.  LEVEL_VECTOR_OUTCOME
// (the outcome at a vector level) stages d as LEVEL_VECTOR does and evaluates g_ji and h only.  A kernel supplies
//   stage_level(g, t, wt)   what rr_ / rc_ hold for individual g (any g: the kernel decides what the padding gets) with
//                           T_g = t (0.0 on the padding), wt = 1 / tyLS^2
//   emit(rp, cq, inside, diag, Bv, terms)   element (row rp, column cq) of the tile: inside = both individuals < n, diag = on the
//                           matrix diagonal, padding included; with level terms, Bv and the terms of an element outside
//                           arrive as 0.0 (g_ji as staged).  Every element depends on its own row and column only.
// ---------------------------------------------------------------------------------------
enum { LEVEL_NONE, LEVEL_SCALAR, LEVEL_VECTOR, LEVEL_VECTOR_OUTCOME };
struct LevelTerms { double e, gij, gji, h; };
template <bool VEC>
__device__ __forceinline__ LevelTerms level_terms(double ti, double tj, double xi, double xj, double wt) {
    const double e = gp_rho(ti, tj, wt);
    if (VEC) return {e, gp_rho(ti, xj, wt), gp_rho(tj, xi, wt), gp_rho(xi, xj, wt)};
    return {e, xi, xj, 1.0};
}
__device__ __forceinline__ LevelTerms level_terms_outcome(double tj, double xi, double xj, double wt) {
    return {0.0, 0.0, gp_rho(tj, xi, wt), gp_rho(xi, xj, wt)};
}
// LDS (doubles): fr [F][128] | fc [F][128] row / column features / LS | tr [128] | tc [128] T | rr_ [128] | rc_ [128]
constexpr int tile_build_lds_bytes(int F) { return (2 * F * GP_TS + 4 * GP_TS) * 8; }

template <int LEVEL, typename StageLevel, typename Emit>
__device__ __forceinline__ void tile_build_body(const SampleGrid& a, long long s, int ti, int tj, double* sm,
                                                StageLevel&& stage_level, Emit&& emit) {
    const int F = a.nU + a.nX;
    double* fr = sm;
    double* fc = fr + F * GP_TS;
    double* tr = fc + F * GP_TS;
    double* tc = tr + GP_TS;
    double* rr_ = tc + GP_TS;
    double* rc_ = rr_ + GP_TS;
    const int tid = threadIdx.x;
    const int n = a.n;
    const int gi0 = ti * GP_TS, gj0 = tj * GP_TS;
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    stage_scaled_features<GP_TS>(a, s, F, F, gi0, fr);
    stage_scaled_features<GP_TS>(a, s, F, F, gj0, fc);
    if (tid < GP_TS) {
        const double t1 = (gi0 + tid < n) ? a.T[gi0 + tid] : 0.0;
        const double t2 = (gj0 + tid < n) ? a.T[gj0 + tid] : 0.0;
        tr[tid] = t1; tc[tid] = t2;
        if (LEVEL != LEVEL_NONE) rr_[tid] = stage_level(gi0 + tid, t1, wt);
        rc_[tid] = stage_level(gj0 + tid, t2, wt);
    }
    __syncthreads();
    const double ys = a.p.yScale[s];
    const int ty = tid & 15, tx = tid >> 4;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const int cq = 8 * tx + q;
        const int gj = gj0 + cq;
        double lux[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) lux[p] = 0.0;
        for (int f = 0; f < F; ++f) {
            const double c = fc[f * GP_TS + cq];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const double d = fr[f * GP_TS + ty + 16 * p] - c;
                lux[p] = fma(d, d, lux[p]);
            }
        }
        const double tcq = tc[cq], xj = rc_[cq];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rp = ty + 16 * p;
            const int gi = gi0 + rp;
            const bool inside = (gi < n) && (gj < n);
            double Bv = 0.0;
            LevelTerms t{0.0, 0.0, xj, 0.0};
            // The level terms stay under this branch: evaluated unconditionally, the eight rows' exp chains of a column
            // interleave and the kernel no longer fits 8 waves per SIMD.  Contrasts (one exp per element) fit without it.
            if (LEVEL == LEVEL_NONE || inside) {
                Bv = ys * gp_exp_neg(-lux[p]);
                if constexpr (LEVEL == LEVEL_VECTOR_OUTCOME) t = level_terms_outcome(tcq, rr_[rp], xj, wt);
                else if constexpr (LEVEL != LEVEL_NONE) t = level_terms<LEVEL == LEVEL_VECTOR>(tr[rp], tcq, rr_[rp], xj, wt);
            }
            emit(rp, cq, inside, gi == gj, Bv, t);
        }
    }
}

// ---------------------------------------------------------------------------------------
// dt_build: tiles of D (D_ij = B_ij (r_j - e_ij), src/estimation.jl:46 "CovWWs' - CovWW") into the
// rectangular matrix W and Delta + pred_noise*I (Delta_ij = B_ij (e_ij - r_i - r_j + 1) =
// CovWW - CovWWs - CovWWs' + CovWsWs, src/likelihood.jl:46-49 / estimation.jl:47, :82) into Cm, with the identity on the padding.
// VEC (per-individual intervention d, k_vec.hip): D_ij = B_ij (g_ji - e_ij), Delta_ij = B_ij (e_ij - g_ij - g_ji + h_ij).
// Without a factual term (FORM is DtArgs::lv.form, level_form.h): at a scalar level D_ij = B_ij cross_j (rc_ holds cross) and
// Delta_ij = B_ij prior — exactly 0 for a contrast with a == b; with VEC D_ij = B_ij g_ji and Delta_ij = B_ij h_ij.
// ---------------------------------------------------------------------------------------
template <bool VEC, int FORM = FORM_ORDINARY>
__global__ __launch_bounds__(256) void dt_build_kernel(DtArgs a) {
    using LF = LevelForm<FORM>;
    constexpr bool NOLV = !LF::factual && !VEC;      // the column block's staged values are all an element needs
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int ti = blockIdx.x / a.nt, tj = blockIdx.x % a.nt;
    const long long b = blockIdx.y, s = a.s0 + b / a.lc;       // batch element = (sample, level) pair
    const int l = a.l0 + (int)(b % a.lc), n = a.n;
    const double doT = VEC ? 0.0 : a.lv.doT[l], doTb = LF::paired ? a.lv.base[l] : 0.0;
    const double* dv = VEC ? a.lv.doT + (long long)n * l : nullptr;
    double kss = 0.0;       // Delta_ij = B_ij kss
    if constexpr (NOLV) {
        const double tl = a.p.tyLS[s];
        const double wt = 1.0 / (tl * tl);
        kss = LF::prior(LF::paired ? gp_rho(doT, doTb, wt) : 0.0, wt);
    }
    double* wt_tile = tref_tile(a.W, b, ti, tj);
    double* c_tile = (ti >= tj) ? tref_tile(a.Cm, b, ti, tj) : nullptr;
    tile_build_body<NOLV ? LEVEL_NONE : !VEC ? LEVEL_SCALAR : LF::factual ? LEVEL_VECTOR : LEVEL_VECTOR_OUTCOME>(
        a, s, ti, tj, sm,
        [&](int g, double t, double wt) {
            if constexpr (VEC) return g < n ? dv[g] : 0.0;
            else return LF::cross(t - doT, gp_rho(t, doT, wt), LF::paired ? gp_rho(t, doTb, wt) : 0.0, wt);
        },
        [&](int rp, int cq, bool inside, bool diag, double Bv, const LevelTerms& t) {
            double Dv, Cv;
            if constexpr (!LF::factual) {
                Dv = Bv * t.gji;
                Cv = VEC ? Bv * t.h : Bv * kss;
            } else {
                Dv = Bv * (t.gji - t.e);
                Cv = Bv * (((t.e - t.gij) - t.gji) + t.h);
            }
            if (!inside) { Dv = 0.0; Cv = diag ? 1.0 : 0.0; }
            else if (diag) Cv += a.pred_noise;
            wt_tile[cq * GP_TS + rp] = Dv;
            if (c_tile) c_tile[cq * GP_TS + rp] = Cv;
        });
}

template <bool VEC, int FORM = FORM_ORDINARY>
static void launch_dt_build_t(const DtArgs& a, int nbatch, hipStream_t st) {
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)dt_build_kernel<VEC, FORM>, tile_build_lds_bytes(MAXF));
    hipLaunchKernelGGL((dt_build_kernel<VEC, FORM>), dim3(a.nt * a.nt, nbatch), dim3(256), tile_build_lds_bytes(a.nU + a.nX), st, a);
}
void launch_dt_build(const DtArgs& a, int nbatch, hipStream_t st) {
    dispatch_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        if (!a.lv.vec) launch_dt_build_t<false, FORM>(a, nbatch, st);
        else if constexpr (LevelForm<FORM>::vector_levels) launch_dt_build_t<true, FORM>(a, nbatch, st);
        else throw std::logic_error("this level form has no vector-level kernels");     // run_predict refuses the call
    });
}

// CovITEs[s + S*(i + n*j)] (src/estimation.jl:75, :82 layout: sample index fastest), both triangles
__global__ __launch_bounds__(256) void gather_cov_kernel(GatherCovArgs a) {
    int ti, tj;
    tri_decode(blockIdx.x, ti, tj);
    const long long b = blockIdx.y, s = a.s0 + b;
    const double* t = tref_tile(a.Cm, b, ti, tj);
    for (int idx = threadIdx.x; idx < GP_TSQ; idx += 256) {
        const int c = idx >> 7, r = idx & 127;
        const long long gi = (long long)ti * GP_TS + r, gj = (long long)tj * GP_TS + c;
        if (gi >= a.n || gj >= a.n || gi < gj) continue;
        const double v = t[idx];
        a.out[s + a.S * (gi + a.n * gj)] = v;
        a.out[s + a.S * (gj + a.n * gi)] = v;
    }
}
void launch_gather_cov(const GatherCovArgs& a, int nbatch, hipStream_t st) {
    hipLaunchKernelGGL(gather_cov_kernel, dim3(a.nt * (a.nt + 1) / 2, nbatch), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------
// likelihoodDistribution blocks (src/likelihood.jl:24-39): K = B.*E, Ks = diag(r) B, Ks' = B diag(r), Kss = B
// VEC (per-individual intervention d): Ks = B.*G, Ks' = B.*G', Kss = B.*H with G_ij = g_ij, H_ij = h_ij of tile_build_body.
// Zeros on the padding.
// ---------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void ld_build_kernel(LdBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int ti = blockIdx.x / a.nt, tj = blockIdx.x % a.nt;
    const int n = a.n;
    double* tK = tref_tile(a.K, 0, ti, tj);
    double* tKs = tref_tile(a.Ks, 0, ti, tj);
    double* tKsT = tref_tile(a.KsT, 0, ti, tj);
    double* tKss = tref_tile(a.Kss, 0, ti, tj);
    tile_build_body<VEC ? LEVEL_VECTOR : LEVEL_SCALAR>(
        a, a.s0, ti, tj, sm,
        [&](int g, double t, double wt) {
            if constexpr (VEC) return g < n ? a.doTv[g] : 0.0;
            else return gp_rho(t, a.doT, wt);
        },
        [&](int rp, int cq, bool inside, bool, double Bv, const LevelTerms& t) {
            const int idx = cq * GP_TS + rp;
            tK[idx] = inside ? Bv * t.e : 0.0;
            tKs[idx] = inside ? t.gij * Bv : 0.0;
            tKsT[idx] = inside ? Bv * t.gji : 0.0;
            tKss[idx] = inside ? Bv * t.h : 0.0;
        });
}
template <bool VEC>
static void launch_ld_build_t(const LdBuildArgs& a, hipStream_t st) {
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)ld_build_kernel<VEC>, tile_build_lds_bytes(MAXF));
    hipLaunchKernelGGL(ld_build_kernel<VEC>, dim3(a.nt * a.nt), dim3(256), tile_build_lds_bytes(a.nU + a.nX), st, a);
}
void launch_ld_build(const LdBuildArgs& a, hipStream_t st) {
    if (a.doTv) launch_ld_build_t<true>(a, st);
    else launch_ld_build_t<false>(a, st);
}

__global__ __launch_bounds__(256) void rect_gather_kernel(RectGatherArgs a) {
    const int ti = blockIdx.x / a.nt, tj = blockIdx.x % a.nt;
    const double* t = tref_tile(a.R, 0, ti, tj);
    for (int idx = threadIdx.x; idx < GP_TSQ; idx += 256) {
        const int c = idx >> 7, r = idx & 127;
        const long long gi = (long long)ti * GP_TS + r, gj = (long long)tj * GP_TS + c;
        if (gi < a.n && gj < a.n) a.out[gi + (long long)a.n * gj] = t[idx] + (gi == gj ? a.diag_add : 0.0);
    }
}
void launch_rect_gather(const RectGatherArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rect_gather_kernel, dim3(a.nt * a.nt), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------
// summarizeEstimates: one workgroup per individual.  The row is gathered into LDS (padded with +inf to a
// power of two), sorted with a bitonic network, and the two order statistics are interpolated exactly as
// Julia's Statistics.quantile does (type 7: aleph = m p + (1 - p), j = trunc(aleph), a + gamma (b - a)).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double julia_quantile_sorted(const double* v, int m, double p) {
#pragma clang fp contract(off)   // Julia evaluates these expressions without fused multiply-adds
    if (m == 1) return v[0];
    const double aleph = (double)m * p + (1.0 - p);
    int j = (int)aleph;                       // trunc
    j = min(max(j, 1), m - 1);
    double gam = aleph - (double)j;
    gam = fmin(fmax(gam, 0.0), 1.0);
    const double a = v[j - 1], b = v[j];
    return a + gam * (b - a);
}

__global__ __launch_bounds__(256) void summarize_kernel(SummArgs a) {
    extern __shared__ __attribute__((aligned(16))) double v[];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long long i = blockIdx.x;
    double acc = 0.0;
    for (int j = tid; j < a.mpad; j += 256) {
        double x = INFINITY;
        if (j < a.m) { x = a.x[i * a.rs + (long long)j * a.cs]; acc += x; }
        v[j] = x;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    const double total = (red[0] + red[1]) + (red[2] + red[3]);
    for (int k = 2; k <= a.mpad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < a.mpad; t += 256) {
                const int u = t ^ j;
                if (u > t) {
                    const bool up = (t & k) == 0;
                    const double p = v[t], q = v[u];
                    if ((p > q) == up) { v[t] = q; v[u] = p; }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        a.mean[i] = total / (double)a.m;
        a.lower[i] = julia_quantile_sorted(v, a.m, a.lowerQ);
        a.upper[i] = julia_quantile_sorted(v, a.m, a.upperQ);
    }
}
// Rows longer than one LDS image (m > 16384: S * spp of a BASELINE-size posterior): exact order statistics by radix
// select on order-preserving 64-bit keys instead of a sort.  One workgroup = 16 consecutive individuals (for the
// column-major n x m sample matrix a wave then reads whole 128-byte lines: 16 rows x 4 samples), thread (r, jj) walks
// samples jj, jj + 16, ... of row r.  Eight passes of 8-bit digits from the top; both quantiles' selections run in the
// same pass (two histograms per row in LDS, ds_add_u32); a ninth pass finds the successor of each selected element
// (count of keys <= it, minimum key above it).  Julia's type-7 interpolation as in julia_quantile_sorted.
#define SUMM_RW 16
__device__ __forceinline__ unsigned long long summ_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double summ_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__global__ __launch_bounds__(256) void summarize_select_kernel(SummArgs a) {
    __shared__ unsigned int hist[SUMM_RW][2][256];
    __shared__ unsigned long long prefix[SUMM_RW][2], mingt[SUMM_RW][2];
    __shared__ unsigned int rank[SUMM_RW][2], cntle[SUMM_RW][2];
    __shared__ double rsum[4][SUMM_RW];
    const int tid = threadIdx.x, r = tid & (SUMM_RW - 1), jj = tid >> 4;
    const long long i = (long long)blockIdx.x * SUMM_RW + r;
    const bool live = i < a.n;
    const double* row = a.x + (live ? i : 0) * a.rs;
    const int m = a.m;
    // ranks (0-based) of the lower neighbour of each quantile: j - 1 with j = clamp(trunc(m p + 1 - p), 1, m - 1)
    int jq[2];
    double gq[2];
    {
#pragma clang fp contract(off)
        const double ps[2] = {a.lowerQ, a.upperQ};
        for (int q = 0; q < 2; ++q) {
            const double aleph = (double)m * ps[q] + (1.0 - ps[q]);
            int j = (int)aleph;
            j = min(max(j, 1), m - 1);
            jq[q] = j;
            gq[q] = fmin(fmax(aleph - (double)j, 0.0), 1.0);
        }
    }
    for (int t = tid; t < SUMM_RW * 2 * 256; t += 256) (&hist[0][0][0])[t] = 0u;
    if (tid < SUMM_RW * 2) {
        const int rr = tid & (SUMM_RW - 1), q = tid >> 4;
        prefix[rr][q] = 0ull; rank[rr][q] = (unsigned)(jq[q] - 1); cntle[rr][q] = 0u; mingt[rr][q] = ~0ull;
    }
    // mean: per-thread strided partial, then the 4 samples-lanes of a wave, then the 4 waves
    double acc = 0.0;
    if (live)
        for (int j = jj; j < m; j += 16) acc += row[(long long)j * a.cs];
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    if ((tid & 63) < SUMM_RW) rsum[tid >> 6][r] = acc;
    __syncthreads();
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (live) {
            const unsigned long long p0 = prefix[r][0], p1 = prefix[r][1];
            for (int j = jj; j < m; j += 16) {
                const unsigned long long k = summ_key(row[(long long)j * a.cs]);
                const unsigned long long hi = pass == 0 ? 0ull : (k >> (shift + 8));
                const unsigned d = (unsigned)(k >> shift) & 255u;
                if (hi == p0) atomicAdd(&hist[r][0][d], 1u);
                if (hi == p1) atomicAdd(&hist[r][1][d], 1u);
            }
        }
        __syncthreads();
        if (tid < SUMM_RW * 2) {
            const int rr = tid & (SUMM_RW - 1), q = tid >> 4;
            unsigned cum = 0, want = rank[rr][q], d = 0;
            for (; d < 255u; ++d) {
                const unsigned cnt = hist[rr][q][d];
                if (want < cum + cnt) break;
                cum += cnt;
            }
            prefix[rr][q] = (prefix[rr][q] << 8) | d;
            rank[rr][q] = want - cum;
        }
        __syncthreads();
        for (int t = tid; t < SUMM_RW * 2 * 256; t += 256) (&hist[0][0][0])[t] = 0u;
        __syncthreads();
    }
    // successor of each selected element
    if (live) {
        const unsigned long long k0 = prefix[r][0], k1 = prefix[r][1];
        unsigned c0 = 0, c1 = 0;
        unsigned long long g0 = ~0ull, g1 = ~0ull;
        for (int j = jj; j < m; j += 16) {
            const unsigned long long k = summ_key(row[(long long)j * a.cs]);
            if (k <= k0) ++c0; else g0 = k < g0 ? k : g0;
            if (k <= k1) ++c1; else g1 = k < g1 ? k : g1;
        }
        atomicAdd(&cntle[r][0], c0); atomicAdd(&cntle[r][1], c1);
        atomicMin(&mingt[r][0], g0); atomicMin(&mingt[r][1], g1);
    }
    __syncthreads();
    if (tid < SUMM_RW && i < a.n) {
#pragma clang fp contract(off)
        double qv[2];
        for (int q = 0; q < 2; ++q) {
            const double av = summ_unkey(prefix[r][q]);                  // sorted[j - 1]
            const double bv = cntle[r][q] > (unsigned)jq[q] ? av : summ_unkey(mingt[r][q]);   // sorted[j]
            qv[q] = m == 1 ? av : av + gq[q] * (bv - av);
        }
        a.mean[i] = ((rsum[0][r] + rsum[1][r]) + (rsum[2][r] + rsum[3][r])) / (double)m;
        a.lower[i] = qv[0];
        a.upper[i] = qv[1];
    }
}

void launch_summarize(const SummArgs& a, hipStream_t st) {
    if (a.m > 16384) {
        hipLaunchKernelGGL(summarize_select_kernel, dim3((a.n + SUMM_RW - 1) / SUMM_RW), dim3(256), 0, st, a);
        return;
    }
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)summarize_kernel, 16384 * 8);
    hipLaunchKernelGGL(summarize_kernel, dim3(a.n), dim3(256), (size_t)a.mpad * 8, st, a);
}
