// The pair product on the MFMA: (B X)[i, col] = sum_j B_ij X[j, col] (and (K X) with K = B .* e) for one row block of 128
// individuals of one posterior sample, B = yScale exp(Lu + Lx), e_ij = exp(-(T_i - T_j)^2 / tyLS^2).  The one body of
// ite_mean_mfma_kernel (k_solve.hip: X[j, l] = r_j(l) alpha_j) and wsum_mfma_kernel (k_wsum.hip: X[j, g] = W[j, g]); DESIGN.md,
// "MeanITE on the MFMA" and §13.  k_new.hip runs it with the new individuals on one side or on both (§19, §25).
//
// No operand tile of B goes through LDS: the f64 16x16x4 MFMA wants one element per lane, and each lane computes exactly its
// own B_rc (row = 16m + lane&15, column = 4kk + lane>>4) from the staged features; the N x ncols right operand is staged per
// 64-column chunk.  One workgroup of 256 threads = 128 rows x passes of up to 64 right-operand columns; wave w owns rows
// 32w..32w+31 (2 row sub-tiles x 4 column sub-tiles = 8 accumulators, 16 with K).  A caller supplies two things:
//   stage_x(j, col, wt, etab)  the value X[j, col] of individual j < n and a live column (wt = 1 / tyLS^2, etab = the staged
//                              exp table); everything else of the chunk is staged as 0.0
//   store(gi, col0, ncol, accB, accK)  the accumulators of one 16-row sub-tile, global row gi (any gi < Np: the caller decides
//                              what rows >= n get), pass origin col0 and ncol live columns; pair_mfma_each_column maps them
//                              to columns.  Per-row work (loads of row gi) belongs here, once per sub-tile.
// What every caller's results rest on lives here once:
//   - B_rc and e_rc are evaluated as gram_kernel evaluates them ((x/l - x'/l)^2 summed by fma in feature order, the
//     table-driven exp, e = 1 or exp(-1/tyLS^2) for binary treatments, B * e in fp64): K X refers to the K that is factorised.
//   - The B and the K accumulation are the same MFMA sequence on the same staged X, so e == 1 everywhere (all T equal) gives
//     K X == B X bit for bit — the exact zeros of the "T == doT" identities rest on it.
//   - Fixed summation order (chunks of 64 individuals in ascending order, four per MFMA): a result does not depend on the
//     batch, the stream or the schedule.
//   - Individuals j >= n are staged with zero features (their B_rc is finite) and X = 0.0.
//   - FREG > 0 keeps this lane's two rows' features in registers, F <= FREG; the features F..FREG-1 are zeros on both sides and
//     add fma(0 - 0, 0 - 0, lux) = lux (lux >= +0) to a pair: the ladder below only has to cover F, and which rung serves an F
//     cannot change a bit.
#pragma once
#include "gpslc_internal.h"
#include "gp_math.h"
#include <type_traits>

constexpr int PM_CC = 64;     // individuals j per staged chunk
constexpr int PM_RLD = 80;    // padded row of the X chunk (doubles): conflict-free ds_read_b64 across the four k rows
constexpr int PM_NL = 64;     // right-operand columns per pass

// LDS (doubles): etab [32] | fr [F][128] row features / LS | fc [FS][PM_CC] column features / LS, FS = max(F, FREG) |
// X [PM_CC][PM_RLD] | with_T: tc [PM_CC] T of the column chunk
constexpr int pair_mfma_lds_bytes(int F, int FS, bool with_T) {
    return (GP_EXP_TAB_DOUBLES + F * GP_TS + FS * PM_CC + PM_CC * PM_RLD + (with_T ? PM_CC : 0)) * 8;
}

// registers for the features of a lane's rows: exact for the common widths, 0 = read them from LDS
template <typename Fn> static void pair_mfma_freg_ladder(int F, Fn&& fn) {
    if (F <= 4) fn(std::integral_constant<int, 4>{});
    else if (F <= 6) fn(std::integral_constant<int, 6>{});
    else if (F <= 8) fn(std::integral_constant<int, 8>{});
    else if (F <= 10) fn(std::integral_constant<int, 10>{});
    else if (F <= 12) fn(std::integral_constant<int, 12>{});
    else fn(std::integral_constant<int, 0>{});
}

// one instantiation's launch: dim3(nt, nbatch) x 256 with the layout's bytes, opted in once per device for F = MAXF
template <auto Kernel, int FREG, bool WITH_T, typename Args>
static void pair_mfma_launch(const Args& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)Kernel, pair_mfma_lds_bytes(MAXF, MAXF, WITH_T));
    hipLaunchKernelGGL(Kernel, dim3(a.nt, nbatch), dim3(256), pair_mfma_lds_bytes(F, FREG > F ? FREG : F, WITH_T), st, a);
}

// acc[q][v] of a 16-row sub-tile is column 16q + (lane >> 4) + 4v of the pass: f(q, v, column) for the live ones
template <typename Fn> __device__ __forceinline__ void pair_mfma_each_column(int ncol, Fn&& f) {
    const int lq = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int ll = 16 * q + lq + 4 * v;
            if (ll < ncol) f(q, v, ll);
        }
}

// stage_rows(F, g0, fr): the features / LS of the 128 rows from g0 into fr [F][128], zeros beyond the row source's end.
// stage_cols(F, FS, c0, fc): those of the PM_CC individuals from c0 on the column side into fc [FS][PM_CC], zeros beyond that
// side's end and in the rows F .. FS - 1; the column side has n individuals, padded to Np (a multiple of PM_CC).  Rows and columns
// may come from different sets of individuals (k_new.hip: the new individuals and the training grid, either way round, or the
// new individuals on both sides) — then WK must be false: e_rc needs both sides' T from `a`.  Row block = blockIdx.x.
template <int FREG, bool WK, int BIN, typename StageRows, typename StageCols, typename StageX, typename Store>
__device__ __forceinline__ void pair_mfma_body_sides(const SampleGrid& a, long long s, int ncols, double* sm, int n, int Np,
                                                     StageRows&& stage_rows, StageCols&& stage_cols, StageX&& stage_x, Store&& store) {
    const int F = a.nU + a.nX;
    double* etab = sm;                       // [32] 2^(j/32): table-driven exp (gp_math.h)
    double* fr = etab + GP_EXP_TAB_DOUBLES;
    const int FS = FREG > F ? FREG : F;      // staged column-feature rows (zero beyond F)
    double* fc = fr + F * GP_TS;
    double* X = fc + FS * PM_CC;
    double* tc = X + PM_CC * PM_RLD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int ib = blockIdx.x;

    stage_rows(F, ib * GP_TS, fr);
    const double ys = a.p.yScale[s];
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    gp_exp_tab_stage(etab, tid);
    const int r0 = 32 * wave + li;           // this lane's rows: r0 and r0 + 16
    const int gr0 = ib * GP_TS + r0, gr1 = gr0 + 16;
    const double tr0 = (WK && gr0 < n) ? a.T[gr0] : 0.0, tr1 = (WK && gr1 < n) ? a.T[gr1] : 0.0;
    __syncthreads();
    const double ew = (WK && BIN) ? gp_exp_neg_tab(-wt, etab) : 0.0;     // e_ij for |T_i - T_j| = 1 (binary treatments)
    double af0[FREG > 0 ? FREG : 1], af1[FREG > 0 ? FREG : 1];
    if (FREG > 0) {
#pragma unroll
        for (int f = 0; f < FREG; ++f) {
            af0[f] = (f < F) ? fr[f * GP_TS + r0] : 0.0;
            af1[f] = (f < F) ? fr[f * GP_TS + r0 + 16] : 0.0;
        }
    }

    for (int l0 = 0; l0 < ncols; l0 += PM_NL) {
        const int nl = min(PM_NL, ncols - l0);
        const int nq = (nl + 15) >> 4;          // live 16-column sub-tiles of this pass (wave-uniform)
        d4 accB[2][4], accK[WK ? 2 : 1][WK ? 4 : 1];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                accB[m][q] = (d4){0.0, 0.0, 0.0, 0.0};
                if constexpr (WK) accK[m][q] = (d4){0.0, 0.0, 0.0, 0.0};
            }
        for (int c0 = 0; c0 < Np; c0 += PM_CC) {
            __syncthreads();
            stage_cols(F, FS, c0, fc);
            if (WK && tid < PM_CC) tc[tid] = (c0 + tid < n) ? a.T[c0 + tid] : 0.0;
            for (int idx = tid; idx < PM_CC * PM_NL; idx += 256) {
                const int cc = idx >> 6, ll = idx & 63;      // consecutive threads -> consecutive right-operand columns
                const int g = c0 + cc;
                X[cc * PM_RLD + ll] = (ll < nl && g < n) ? stage_x(g, l0 + ll, wt, etab) : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < PM_CC / 4; ++kk) {
                const int cc = 4 * kk + lq;            // this lane's column inside the chunk
                double lux0 = 0.0, lux1 = 0.0;
                if (FREG > 0) {
#pragma unroll
                    for (int f = 0; f < FREG; ++f) {       // fc rows beyond F are zero-filled
                        const double cf = fc[f * PM_CC + cc];
                        const double d0 = af0[f] - cf, d1 = af1[f] - cf;
                        lux0 = fma(d0, d0, lux0);
                        lux1 = fma(d1, d1, lux1);
                    }
                } else {
                    for (int f = 0; f < F; ++f) {
                        const double cf = fc[f * PM_CC + cc];
                        const double d0 = fr[f * GP_TS + r0] - cf;
                        const double d1 = fr[f * GP_TS + r0 + 16] - cf;
                        lux0 = fma(d0, d0, lux0);
                        lux1 = fma(d1, d1, lux1);
                    }
                }
                const double B0 = ys * gp_exp_neg_tab(-lux0, etab), B1 = ys * gp_exp_neg_tab(-lux1, etab);
                double K0 = 0.0, K1 = 0.0;
                if constexpr (WK) {
                    const double tcc = tc[cc];
                    const double t0 = tr0 - tcc, t1 = tr1 - tcc;
                    const double E0 = BIN ? (t0 == 0.0 ? 1.0 : ew) : gp_exp_neg_tab(-((t0 * t0) * wt), etab);
                    const double E1 = BIN ? (t1 == 0.0 ? 1.0 : ew) : gp_exp_neg_tab(-((t1 * t1) * wt), etab);
                    K0 = B0 * E0; K1 = B1 * E1;
                }
                const double* Xrow = X + cc * PM_RLD + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < nq) {
                        const double xf = Xrow[16 * q];
                        accB[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, B0, accB[0][q], 0, 0, 0);
                        accB[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, B1, accB[1][q], 0, 0, 0);
                        if constexpr (WK) {
                            accK[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, K0, accK[0][q], 0, 0, 0);
                            accK[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, K1, accK[1][q], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // acc[m][q][v] = (B X)[row 32w + 16m + li][column l0 + 16q + lq + 4v]
#pragma unroll
        for (int m = 0; m < 2; ++m) store(ib * GP_TS + 32 * wave + 16 * m + li, l0, nl, accB[m], accK[WK ? m : 0]);
    }
}

// the columns from the training grid, the rows from stage_rows (new_mean_mfma_kernel: the new individuals)
template <int FREG, bool WK, int BIN, typename StageRows, typename StageX, typename Store>
__device__ __forceinline__ void pair_mfma_body_rows(const SampleGrid& a, long long s, int ncols, double* sm, StageRows&& stage_rows,
                                                    StageX&& stage_x, Store&& store) {
    pair_mfma_body_sides<FREG, WK, BIN>(
        a, s, ncols, sm, a.n, a.nt * GP_TS, stage_rows,
        [&](int F, int FS, int c0, double* fc) { stage_scaled_features<PM_CC>(a, s, F, FS, c0, fc); }, stage_x, store);
}

// rows and columns from the same grid: the body of ite_mean_mfma_kernel and wsum_mfma_kernel
template <int FREG, bool WK, int BIN, typename StageX, typename Store>
__device__ __forceinline__ void pair_mfma_body(const SampleGrid& a, long long s, int ncols, double* sm, StageX&& stage_x,
                                               Store&& store) {
    pair_mfma_body_rows<FREG, WK, BIN>(
        a, s, ncols, sm, [&](int F, int g0, double* fr) { stage_scaled_features<GP_TS>(a, s, F, F, g0, fr); }, stage_x, store);
}
