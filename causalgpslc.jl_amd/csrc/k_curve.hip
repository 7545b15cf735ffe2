// Joint covariance of the weighted effects of one call across its levels: for weight column w_g, posterior
// sample s and levels l, l' with tau_l = w_g' ITE_l,
//
//     Cov(tau_l, tau_l') = P_ll' - v_l . v_l' + [l == l'] pred_noise (w . w)
//
// v_q = L^-1 c_q are the right-hand-side rows the factorisation has carried (row q = 1 + l + L*g of the augmented tiles) and
// P the prior term: with bw = B w, kw = K w (k_wsum.hip), beta = w . bw, kappa = w . kw, gamma_l = sum_j w_j r^l_j bw_j and
// rho(x, y) = exp(-(x - y)^2 / tyLS^2)
//     P_ll' = joint_ll' beta                                the forms without a factual term (joint: level_form.h)
//     P_ll' = rho(d_l, d_l') beta - gamma_l - gamma_l' + kappa    the factual form, f(d_l) - f(T)
//
//   curve_prior_kernel   beta (and, factual, kappa, gamma_l) per (sample, weight column): fixed trees over the threads' strided j
//   curve_gram_kernel    one workgroup per (16 x 16 block of right-hand-side pairs, sample): v_q . v_q' with
//                        v_mfma_f64_16x16x4_f64 straight from the augmented rows, then P - Gram for l' < l, written to both
//                        triangles; the diagonal is the value the epilogue stored as varW
#include "gpslc_internal.h"
#include "gp_math.h"

// grid (G, batch).  prior[b][g][0] = beta, [1] = kappa, [2 + l] = gamma_l; without a factual term beta alone (kw is not
// computed then and is not read)
template <bool FACTUAL>
__global__ __launch_bounds__(256) void curve_prior_kernel(CurveArgs a) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int g = blockIdx.x, b = blockIdx.y;
    const long long s = a.s0 + b;
    const int Np = a.nt * GP_TS;
    const double* bs = a.bw + ((long long)b * a.G + g) * Np;
    const double* ks = a.kw + ((long long)b * a.G + g) * Np;
    double* out = a.prior + ((long long)b * a.G + g) * (a.lv.L + 2);
    double ab = 0.0, ak = 0.0;
    for (int j = tid; j < a.n; j += 256) {
        const double w = a.W[(long long)j * a.G + g];
        ab = fma(w, bs[j], ab);
        if (FACTUAL) ak = fma(w, ks[j], ak);
    }
    const double beta = block_sum_256(ab, red);
    const double kappa = FACTUAL ? block_sum_256(ak, red) : 0.0;
    if (tid == 0) { out[0] = beta; out[1] = kappa; }
    if (!FACTUAL) return;
    const double tl = a.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    for (int l = 0; l < a.lv.L; ++l) {
        const double dot = a.lv.doT[l];
        double acc = 0.0;
        for (int j = tid; j < a.n; j += 256) {
            const double w = a.W[(long long)j * a.G + g];
            acc = fma(w * gp_rho(a.T[j], dot, wt), bs[j], acc);
        }
        const double gam = block_sum_256(acc, red);
        if (tid == 0) out[2 + l] = gam;
    }
}

// grid (nblk (nblk + 1) / 2, batch), nblk = ceil((R + 1) / 16) blocks of 16 right-hand sides, R = L G.  Workgroup p is the block
// pair (A, Bk), Bk <= A.  Right-hand side q of column i sits at tile (nt + q / 128, i / 128)[(i % 128) * 128 + q % 128]: the 16
// q of a block are one 128-byte line per column, so lane (r = lane & 15, k = lane >> 4) loads its MFMA operand — row 16 A + r,
// column 4 kg + k of column group kg — straight from global memory.  Only rows below 16 nblk are read: with <= 32 live rows
// the rest of the augmented tile is undefined (rhs_tiles_kernel).  Wave w takes the column groups w, w + 4, ... of every tile
// column in ascending order, alternating between two accumulators; the four waves' sums meet in LDS as (w0 + w1) + (w2 + w3).
// Accumulator v of a lane is the pair (qa = 16 A + (lane >> 4) + 4 v, qb = 16 Bk + (lane & 15)) (diag_block.h: mma).
template <int FORM>
__global__ __launch_bounds__(256) void curve_gram_kernel(CurveArgs a) {
    using LF = LevelForm<FORM>;
    __shared__ double part[4][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long long s = a.s0 + b;
    const int L = a.lv.L, R = L * a.G;
    int A = 0;
    while ((A + 1) * (A + 2) / 2 <= (int)blockIdx.x) ++A;
    const int Bk = (int)blockIdx.x - A * (A + 1) / 2;
    // no pair of the same weight column in this block pair: the columns of block A start beyond the last column of block Bk
    const int ga_lo = (max(16 * A, 1) - 1) / L, gb_hi = (min(16 * Bk + 15, R) - 1) / L;
    if (gb_hi < ga_lo) return;
    const int lane_off = (lane & 15) + (lane >> 4) * GP_TS;
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int tj = 0; tj < a.nt; ++tj) {
        const double* pa = tref_tile(a.M, b, a.nt + (A >> 3), tj) + (A & 7) * 16 + lane_off;
        const double* pb = tref_tile(a.M, b, a.nt + (Bk >> 3), tj) + (Bk & 7) * 16 + lane_off;
        double av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int col = 4 * (wave + 4 * u);
            av[u] = pa[col * GP_TS];
            bv[u] = pb[col * GP_TS];
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u + 1], bv[u + 1], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) part[wave][v][lane] = acc0[v] + acc1[v];
    __syncthreads();
    // thread -> one pair of the block: v = tid >> 6 of lane tid & 63
    const int qa = 16 * A + (lane >> 4) + 4 * wave, qb = 16 * Bk + (lane & 15);
    if (qa < 1 || qb < 1 || qa > R || qb > qa) return;
    const int g = (qa - 1) / L, l = (qa - 1) - L * g;
    if ((qb - 1) / L != g) return;
    const int lp = (qb - 1) - L * g;                      // l' <= l
    double* cov = a.covW + s + a.S * ((long long)L * L * g);
    if (lp == l) {
        cov[a.S * ((long long)l + (long long)L * l)] = a.varW[s + a.S * ((long long)l + (long long)L * g)];
        return;
    }
    const double gram = (part[0][wave][lane] + part[1][wave][lane]) + (part[2][wave][lane] + part[3][wave][lane]);
    const double* pr = a.prior + ((long long)b * a.G + g) * (L + 2);
    const double tl = a.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    const double x = a.lv.doT[l], xp = a.lv.doT[lp];
    double rab = 0.0, rba = 0.0, rbb = 0.0;
    if constexpr (LF::paired) {
        const double y = a.lv.base[l], yp = a.lv.base[lp];
        rab = gp_rho(x, yp, wt); rba = gp_rho(y, xp, wt); rbb = gp_rho(y, yp, wt);
    }
    double P = LF::joint(gp_rho(x, xp, wt), rab, rba, rbb, x - xp, wt) * pr[0];
    if constexpr (LF::factual) P = ((P - pr[2 + l]) - pr[2 + lp]) + pr[1];
    const double val = P - gram;
    cov[a.S * ((long long)l + (long long)L * lp)] = val;
    cov[a.S * ((long long)lp + (long long)L * l)] = val;
}

template <int FORM>
static void launch_curve_t(const CurveArgs& a, int nbatch, hipStream_t st, bool prior_given) {
    const int nblk = (a.lv.L * a.G + 1 + 15) / 16;
    if (!prior_given) hipLaunchKernelGGL(curve_prior_kernel<LevelForm<FORM>::factual>, dim3(a.G, nbatch), dim3(256), 0, st, a);
    hipLaunchKernelGGL(curve_gram_kernel<FORM>, dim3(nblk * (nblk + 1) / 2, nbatch), dim3(256), 0, st, a);
}
void launch_curve(const CurveArgs& a, int nbatch, hipStream_t st, bool prior_given) {
    dispatch_form(a.lv.form, [&](auto form) { launch_curve_t<decltype(form)::value>(a, nbatch, st, prior_given); });
}
