// Weighted column sums of B and K for group-weighted average effects.
//
//   BW[i, g] = sum_j B_ij W[j, g]        KW[i, g] = sum_j B_ij e_ij W[j, g]
//
// with B = yScale exp(Lu + Lx), e_ij = exp(-(T_i - T_j)^2 / tyLS^2), K = B .* e (B and K are symmetric: these are the
// weighted column sums; W = 1 gives the bsum / ksum of the Gram build).  One workgroup = one row block of 128 individuals of
// one posterior sample, all G weight columns in passes of 64; the shape of ite_mean_mfma_kernel (k_solve.hip): no operand
// tile goes through LDS, each lane computes its own B_rc (row = 16m + lane&15, column = 4kk + lane>>4) from the staged
// features, the N x G right-hand side is staged per 64-column chunk, v_mfma_f64_16x16x4_f64 accumulates.
//
//   - B_rc and e_rc are evaluated as gram_kernel evaluates them ((x/l - x'/l)^2 summed by fma in feature order, the
//     table-driven exp, e = 1 or exp(-1/tyLS^2) for binary treatments, B * e in fp64): KW refers to the K that is factorised.
//   - The B and the K accumulation are the same MFMA sequence on the same staged W, so e == 1 everywhere (all T equal) gives
//     KW == BW bit for bit — the exact zeros of the "T == doT" identities rest on it.
//   - Fixed summation order (chunks of 64 columns in order, four columns per MFMA): a result does not depend on the batch,
//     the stream or the schedule.
//   - Columns j >= n are staged as zero weights (their B_rc is finite: zero features), rows i >= n are written as 0.0.
//   - WK = false (contrasts: c needs no KW): no e, no second MFMA.
#include "gpslc_internal.h"
#include "gp_math.h"

#define WS_CC 64          // columns per staged chunk
#define WS_RLD 80         // padded row of the W chunk (doubles): conflict-free ds_read_b64 across the four k rows
#define WS_NL 64          // weight columns per pass
#define WS_MAXF 32

template <int FREG, bool WK, int BIN>   // FREG > 0: this lane's two rows' features live in registers (F <= FREG); 0: read from LDS
__global__ __launch_bounds__(256, 2) void wsum_mfma_kernel(WsumArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int F = a.nU + a.nX;
    double* etab = sm;                       // [32] 2^(j/32): table-driven exp (gp_math.h)
    double* fr = etab + GP_EXP_TAB_DOUBLES;  // [F][128] row features / LS
    const int FSL = FREG > F ? FREG : F;
    double* fc = fr + F * GP_TS;             // [max(F, FREG)][WS_CC] column features / LS
    double* Wc = fc + FSL * WS_CC;           // [WS_CC][WS_RLD]  W[j, g0 + ll]
    double* tc = Wc + WS_CC * WS_RLD;        // [WS_CC] T of the column chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int ib = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int n = a.n, Np = a.nt * GP_TS, G = a.G;

    auto feat_src = [&](int f) { return a.column(s, f); };
    auto feat_il = [&](int f) { return 1.0 / a.lengthscale(s, f); };
    for (int idx = tid; idx < F * GP_TS; idx += 256) {
        const int f = idx >> 7, rr = idx & 127;
        const int g = ib * GP_TS + rr;
        fr[idx] = (g < n) ? feat_src(f)[g] * feat_il(f) : 0.0;
    }
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

    for (int g0 = 0; g0 < G; g0 += WS_NL) {
        const int ng = min(WS_NL, G - g0);
        const int nq = (ng + 15) >> 4;          // live 16-column sub-tiles of this pass (wave-uniform)
        d4 accB[2][4], accK[WK ? 2 : 1][WK ? 4 : 1];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                accB[m][q] = (d4){0.0, 0.0, 0.0, 0.0};
                if constexpr (WK) accK[m][q] = (d4){0.0, 0.0, 0.0, 0.0};
            }
        for (int c0 = 0; c0 < Np; c0 += WS_CC) {
            __syncthreads();
            const int FS = FREG > F ? FREG : F;      // staged feature rows (zero beyond F)
            for (int idx = tid; idx < FS * WS_CC; idx += 256) {
                const int f = idx / WS_CC, cc = idx - f * WS_CC;
                const int g = c0 + cc;
                fc[idx] = (f < F && g < n) ? feat_src(f)[g] * feat_il(f) : 0.0;
            }
            if (WK && tid < WS_CC) tc[tid] = (c0 + tid < n) ? a.T[c0 + tid] : 0.0;
            for (int idx = tid; idx < WS_CC * WS_NL; idx += 256) {
                const int cc = idx >> 6, ll = idx & 63;      // consecutive threads -> consecutive weight columns (W is g-fastest)
                const int g = c0 + cc;
                Wc[cc * WS_RLD + ll] = (ll < ng && g < n) ? a.W[(long long)g * G + (g0 + ll)] : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < WS_CC / 4; ++kk) {
                const int cc = 4 * kk + lq;            // this lane's column inside the chunk
                double lux0 = 0.0, lux1 = 0.0;
                if (FREG > 0) {
#pragma unroll
                    for (int f = 0; f < FREG; ++f) {       // fc rows beyond F are zero-filled
                        const double cf = fc[f * WS_CC + cc];
                        const double d0 = af0[f] - cf, d1 = af1[f] - cf;
                        lux0 = fma(d0, d0, lux0);
                        lux1 = fma(d1, d1, lux1);
                    }
                } else {
                    for (int f = 0; f < F; ++f) {
                        const double cf = fc[f * WS_CC + cc];
                        const double d0 = fr[f * GP_TS + r0] - cf;
                        const double d1 = fr[f * GP_TS + r0 + 16] - cf;
                        lux0 = fma(d0, d0, lux0);
                        lux1 = fma(d1, d1, lux1);
                    }
                }
                const double B0 = ys * gp_exp_neg_tab(-lux0, etab), B1 = ys * gp_exp_neg_tab(-lux1, etab);
                double K0 = 0.0, K1 = 0.0;
                if (WK) {
                    const double tcc = tc[cc];
                    const double t0 = tr0 - tcc, t1 = tr1 - tcc;
                    const double E0 = BIN ? (t0 == 0.0 ? 1.0 : ew) : gp_exp_neg_tab(-((t0 * t0) * wt), etab);
                    const double E1 = BIN ? (t1 == 0.0 ? 1.0 : ew) : gp_exp_neg_tab(-((t1 * t1) * wt), etab);
                    K0 = B0 * E0; K1 = B1 * E1;
                }
                const double* Wrow = Wc + cc * WS_RLD + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < nq) {
                        const double wf = Wrow[16 * q];
                        accB[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, B0, accB[0][q], 0, 0, 0);
                        accB[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, B1, accB[1][q], 0, 0, 0);
                        if constexpr (WK) {
                            accK[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, K0, accK[0][q], 0, 0, 0);
                            accK[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, K1, accK[1][q], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // acc[m][q][v] = (B W)[row 32w + 16m + li][column 16q + lq + 4v]; bw / kw are [b][G][Np]
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int gi = ib * GP_TS + 32 * wave + 16 * m + li;
            const bool in = gi < n;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int ll = 16 * q + lq + 4 * v;
                    if (ll < ng) {
                        const long long o = (b * G + (g0 + ll)) * Np + gi;
                        a.bw[o] = in ? accB[m][q][v] : 0.0;
                        if constexpr (WK) a.kw[o] = in ? accK[m][q][v] : 0.0;
                    }
                }
        }
    }
}

template <int FREG, bool WK, int BIN>
static void launch_wsum_t(const WsumArgs& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    const int FS = FREG > F ? FREG : F;
    const int bytes = (GP_EXP_TAB_DOUBLES + F * GP_TS + FS * WS_CC + WS_CC * WS_RLD + WS_CC) * 8;
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)wsum_mfma_kernel<FREG, WK, BIN>,
               (GP_EXP_TAB_DOUBLES + WS_MAXF * GP_TS + WS_MAXF * WS_CC + WS_CC * WS_RLD + WS_CC) * 8);
    hipLaunchKernelGGL((wsum_mfma_kernel<FREG, WK, BIN>), dim3(a.nt, nbatch), dim3(256), bytes, st, a);
}
template <bool WK, int BIN>
static void launch_wsum_f(const WsumArgs& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    if (F <= 4) launch_wsum_t<4, WK, BIN>(a, nbatch, st);
    else if (F <= 6) launch_wsum_t<6, WK, BIN>(a, nbatch, st);
    else if (F <= 8) launch_wsum_t<8, WK, BIN>(a, nbatch, st);
    else if (F <= 12) launch_wsum_t<12, WK, BIN>(a, nbatch, st);
    else launch_wsum_t<0, WK, BIN>(a, nbatch, st);
}
void launch_wsum(const WsumArgs& a, int nbatch, hipStream_t st) {
    if (!a.with_k) launch_wsum_f<false, 0>(a, nbatch, st);
    else if (a.binary_t) launch_wsum_f<true, 1>(a, nbatch, st);
    else launch_wsum_f<true, 0>(a, nbatch, st);
}
