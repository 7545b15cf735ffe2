// Predictions for new individuals: mean, variance and covariance of a non-factual level form (level_form.h:
// outcome f*(a), contrast f*(a) - f*(b), slope df*/dt at a) at m individuals that are not in the data, per posterior sample s and
// level l.  With w*_i = [u*_i(s) | x*_i], B*_ij = yScale exp(-sum_f ((w*_if - w_jf) / l_f)^2) (m x n), B** the same between two
// new individuals (m x m), A = K + yNoise I = L L^T and alpha = A^-1 Y from unit A:
//     D*(l) = B* diag(cross(l))      mean(l) = D*(l) alpha = (B* R)[:, l], R[j, l] = cross_j(l) alpha_j      W*(l) = D*(l) L^-T
//     var_i(l) = (prior_l yScale - ||row i of W*(l)||^2) + pred_noise      cov(l) = prior_l B** + pred_noise I - W*(l) W*(l)^T
// Here: the mean on the MFMA (the pair-product body of pair_mfma.h with the rows from the new grid), the builder of the D*(l) and
// prior_l B** tiles, the row norms that give var, and the gather of cov into the caller's layout.  The solve W* = D* L^-T and the
// product W* W*^T are the tile kernels' (w_solve, predict.hip; gemm, factor.hip).
// Every output element depends on its own new individual(s), the training data and the sample only, in a fixed summation order:
// results do not depend on which other new individuals share the call, nor on the chunk, the stream or the schedule.
// Further down: weighted averages over the new individuals, which need none of these tiles; and levels that depend
// on the new individual with the score of a held-out test set on top of them: the mean as a pass over the pairs, the
// VEC instantiations of the builder and of the row norms, the augmented row and the densities of the score.
#include "pair_mfma.h"
#include <stdexcept>

namespace {

// prior_l of batch element (s, l): Delta*_ii' = prior_l B**_ii'
template <int FORM, class Args>
__device__ __forceinline__ double new_prior(const Args& a, long long s, int l) {
    using LF = LevelForm<FORM>;
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    return LF::prior(LF::paired ? gp_rho(a.lv.doT[l], a.lv.base[l], wt) : 0.0, wt);
}

// ---------------------------------------------------------------------------------------
// mean[i, s, l] = sum_j B*_ij cross_j(l) alpha_j for one block of 128 new individuals of one sample and all L levels: what is
// staged is ite_mean_mfma_kernel's R (k_solve.hip), so new individuals that copy training rows reproduce the non-factual MeanITE
// of those rows bit for bit.  A level that is zero by its form (a contrast with a == b) is stored as 0.0.
// ---------------------------------------------------------------------------------------
template <int FREG, int FORM>
__global__ __launch_bounds__(256, 2) void new_mean_mfma_kernel(NewArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    using LF = LevelForm<FORM>;
    const long long b = blockIdx.y, s = a.s0 + b;
    const double* alpha = a.alpha + b * (a.nt * GP_TS);
    const double* doT = a.lv.doT;
    pair_mfma_body_rows<FREG, false, 0>(
        a, s, a.lv.L, sm, [&](int F, int g0, double* fr) { stage_scaled_new_features<GP_TS>(a, s, F, F, g0, fr); },
        [&](int j, int l, double wt, const double* etab) {
            const double dt = a.T[j] - doT[l], db = LF::paired ? a.T[j] - a.lv.base[l] : 0.0;
            const double rb = LF::paired ? gp_exp_neg_tab(-((db * db) * wt), etab) : 0.0;
            return LF::cross(dt, gp_exp_neg_tab(-((dt * dt) * wt), etab), rb, wt) * alpha[j];
        },
        [&](int gi, int l0, int nl, const d4* acc, const d4*) {
            if (gi >= a.m) return;
            double* out = a.mean + gi + (long long)a.m * s;
            pair_mfma_each_column(nl, [&](int q, int v, int ll) {
                out[(long long)a.m * a.S * (l0 + ll)] = (LF::paired && LF::zero_level(doT[l0 + ll], a.lv.base[l0 + ll])) ? 0.0 : acc[q][v];
            });
        });
}

template <int FORM>
void launch_new_mean_t(const NewArgs& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    pair_mfma_freg_ladder(F, [&](auto freg) {
        constexpr int FREG = decltype(freg)::value;
        static DeviceOnce attr_set;
        lds_opt_in(attr_set, (const void*)new_mean_mfma_kernel<FREG, FORM>, pair_mfma_lds_bytes(MAXF, MAXF, false));
        hipLaunchKernelGGL((new_mean_mfma_kernel<FREG, FORM>), dim3(a.mt, nbatch), dim3(256),
                           pair_mfma_lds_bytes(F, FREG > F ? FREG : F, false), st, a);
    });
}

// ---------------------------------------------------------------------------------------
// One workgroup fills one 128 x 128 tile, in the shape of tile_build_body (k_solve.hip: thread (ty, tx) owns rows ty + 16p and
// columns 8 tx + q; (x/l - x'/l)^2 summed by fma in feature order) with the table-driven exp of gram_kernel.  blockIdx.x < mt nt:
// tile (ti, tj) of D*(l), rows = new individuals, columns = training individuals, D*_ij = B*_ij cross_j(l), zeros in the rows
// >= m and the columns >= n (the factor's padding is the identity: the padding of W* stays zero).  Beyond (covariance asked): tile
// (ti, tj), tj <= ti, of prior_l B** + pred_noise I, new individuals on both sides, zeros on the padding.
// A contrast with a == b: cross_j = r^a_j - r^b_j = 0.0 for every j (the same square into the same exp) and prior = 0.0.
// LDS (doubles): etab [32] | fr [F][128] | fc [F][128] | xc [128] cross_j of the column block
// ---------------------------------------------------------------------------------------
// VEC (per-individual levels): xc gives way to ra | rb | ca | cb [128] each, the doses (and baselines) of the row
// block and, for a Cm tile, of the column block; cross_ij and P_ii' are evaluated per element with the table-driven exp (one
// exp per element for the outcome; two for a D* tile and four for a Cm tile of the contrast).  a.score: the padded diagonal of Cm
// is the identity (the tile is factorised); a.noise_s: the sample's yNoise on the diagonal.
constexpr int new_build_lds_bytes(int F, bool vec = false) { return (GP_EXP_TAB_DOUBLES + 2 * F * GP_TS + (vec ? 4 : 1) * GP_TS) * 8; }

template <int FORM, bool VEC>
__global__ __launch_bounds__(256) void new_build_kernel(NewArgs a) {
    using LF = LevelForm<FORM>;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int F = a.nU + a.nX;
    double* etab = sm;
    double* fr = etab + GP_EXP_TAB_DOUBLES;
    double* fc = fr + F * GP_TS;
    double* xc = fc + F * GP_TS;
    const int tid = threadIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b / a.lc;
    const int l = a.l0 + (int)(b % a.lc);
    const int nrect = a.mt * a.nt;
    const bool cross = (int)blockIdx.x < nrect;       // workgroup-uniform
    int ti, tj;
    if (cross) { ti = blockIdx.x / a.nt; tj = blockIdx.x % a.nt; }
    else tri_decode((int)blockIdx.x - nrect, ti, tj);
    const int gi0 = ti * GP_TS, gj0 = tj * GP_TS;
    const int ncol = cross ? a.n : a.m;               // individuals on the column side
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    stage_scaled_new_features<GP_TS>(a, s, F, F, gi0, fr);
    if (cross) stage_scaled_features<GP_TS>(a, s, F, F, gj0, fc);
    else stage_scaled_new_features<GP_TS>(a, s, F, F, gj0, fc);
    gp_exp_tab_stage(etab, tid);
    if (VEC) {       // xc: ra | rb | ca | cb
        for (int idx = tid; idx < 4 * GP_TS; idx += 256) {
            const int k = idx >> 7, r = idx & 127, g = (k < 2 ? gi0 : gj0) + r;
            const double* src = (k & 1) ? a.lv.base : a.lv.doT;
            xc[idx] = (src && g < a.m && (k < 2 || !cross)) ? src[g + (long long)a.m * l] : 0.0;
        }
    } else if (cross && tid < GP_TS) {
        const int g = gj0 + tid;
        double v = 0.0;
        if (g < a.n) {
            const double t = a.T[g], doT = a.lv.doT[l];
            v = LF::cross(t - doT, gp_rho(t, doT, wt), LF::paired ? gp_rho(t, a.lv.base[l], wt) : 0.0, wt);
        }
        xc[tid] = v;
    }
    double prior = 0.0;
    if constexpr (!VEC) prior = cross ? 0.0 : new_prior<FORM>(a, s, l);
    __syncthreads();
    const double ys = a.p.yScale[s];
    const double noise = (VEC && a.noise_s) ? a.noise_s[s] : a.pred_noise;
    auto rho = [&](double x, double y) { const double d = x - y; return gp_exp_neg_tab(-((d * d) * wt), etab); };
    double* tile = tref_tile(cross ? a.W : a.Cm, b, ti, tj);
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
        const double xj = VEC ? 0.0 : cross ? xc[cq] : prior;
        const double tj = (VEC && cross && gj < a.n) ? a.T[gj] : 0.0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rp = ty + 16 * p;
            const int gi = gi0 + rp;
            double v = 0.0;
            if (gi < a.m && gj < ncol) {
                double x = xj;
                if constexpr (VEC) {
                    const double ai = xc[rp], bi = xc[GP_TS + rp];
                    if (cross) x = LF::cross(tj - ai, rho(tj, ai), LF::paired ? rho(tj, bi) : 0.0, wt);
                    else x = level_pair_prior<FORM>(ai, bi, xc[2 * GP_TS + cq], xc[3 * GP_TS + cq], wt, rho);
                }
                v = (ys * gp_exp_neg_tab(-lux[p], etab)) * x;
                if (!cross && gi == gj) v += noise;
            } else if (VEC && !cross && a.score && gi == gj) {
                v = 1.0;
            }
            tile[cq * GP_TS + rp] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// var[i, s, l] = (prior_l yScale - ||row i of W*(l)||^2) + pred_noise: a sum of squares subtracted once.  One workgroup per row
// tile and batch element; summation order of a row, fixed and the same for every row of a tile (loo_rownorm_kernel's): per column
// parity h of the tiles (two halves of the workgroup) ascending k, inside a tile ascending column in four interleaved partial sums
// ((p0 + p1) + (p2 + p3)); the norm = half 0 + half 1.
// ---------------------------------------------------------------------------------------
// VEC: prior_l is the row's own P_ii = prior(rho(a_i, b_i)), and a.noise_s (the test-set score) takes pred_noise's place.
template <int FORM, bool VEC>
__global__ __launch_bounds__(256) void new_var_kernel(NewArgs a) {
    __shared__ double s_half[GP_TS];
    const int i = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b / a.lc;
    const int l = a.l0 + (int)(b % a.lc);
    const int r = threadIdx.x & (GP_TS - 1), h = threadIdx.x >> 7;
    double acc = 0.0;
    for (int k = 0; k < a.nt; ++k) {
        const double* __restrict__ t = tref_tile(a.W, b, i, k) + r;
        double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int q = 0; q < GP_TS / 2; q += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double w = t[(2 * (q + u) + h) * GP_TS];
                p[u] = fma(w, w, p[u]);
            }
        }
        acc += (p[0] + p[1]) + (p[2] + p[3]);
    }
    if (h == 1) s_half[r] = acc;
    __syncthreads();
    const int gi = i * GP_TS + r;
    if (h == 0 && gi < a.m) {
        if constexpr (VEC) {
            using LF = LevelForm<FORM>;
            const double tl = a.p.tyLS[s], wt = 1.0 / (tl * tl);
            const long long o = gi + (long long)a.m * l;
            const double prior = LF::prior(LF::paired ? gp_rho(a.lv.doT[o], a.lv.base[o], wt) : 0.0, wt);
            a.var[gi + (long long)a.m * (s + a.S * l)] = (prior * a.p.yScale[s] - (acc + s_half[r])) + (a.noise_s ? a.noise_s[s] : a.pred_noise);
        } else {
            a.var[gi + (long long)a.m * (s + a.S * l)] = (new_prior<FORM>(a, s, l) * a.p.yScale[s] - (acc + s_half[r])) + a.pred_noise;
        }
    }
}

// cov[i, i', s, l] from the lower tiles of Cm, both triangles from the one value (exactly symmetric); the diagonal is var's value
__global__ __launch_bounds__(256) void new_gather_kernel(NewArgs a) {
    int ti, tj;
    tri_decode(blockIdx.x, ti, tj);
    const long long b = blockIdx.y, s = a.s0 + b / a.lc;
    const int l = a.l0 + (int)(b % a.lc);
    const long long m = a.m;
    const double* t = tref_tile(a.Cm, b, ti, tj);
    const double* var = a.var + m * (s + a.S * l);
    double* out = a.cov + m * m * (s + a.S * l);
    for (int idx = threadIdx.x; idx < GP_TSQ; idx += 256) {
        const int c = idx >> 7, r = idx & 127;
        const long long gi = (long long)ti * GP_TS + r, gj = (long long)tj * GP_TS + c;
        if (gi >= m || gj >= m || gi < gj) continue;
        if (gi == gj) { out[gi + m * gi] = var[gi]; continue; }
        const double v = t[idx];
        out[gi + m * gj] = v;
        out[gj + m * gi] = v;
    }
}

// ---------------------------------------------------------------------------------------
// Weighted averages over the new individuals: tau_g(l) = w_g' f*(l) for G weight columns over the m new
// individuals.  c_g(l) = D*(l)' w_g = cross(l) .* bw*_g with bw*_g = B*' w_g, and w_g' Delta*(l, l') w_g = joint_ll' beta_g with
// beta_g = w_g' B** w_g: with bw*, sumdelta = prior_l beta_g, wnorm2 = w_g . w_g and beta the weighted call's kernels (rhs_tiles,
// the factorisation, the epilogue, curve_gram: §13, §14) do the rest, and neither an mt x nt tile workspace nor anything m x m
// exists.  Both passes are wsum_mfma_kernel's product (k_wsum.hip: X[i, g] = W[i, g], passes of 64 weight columns) with another
// choice of the two sides.
// ---------------------------------------------------------------------------------------
// bw*[j, g] = sum_i B*_ij W[i, g] for one row block of 128 training individuals of one sample: the new individuals are the column
// side.  The store is wsum_mfma_kernel's: new individuals that copy the training individuals give that kernel's bw bit for bit.
template <int FREG>
__global__ __launch_bounds__(256, 2) void new_wsum_cross_kernel(NewWsumArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const long long b = blockIdx.y, s = a.s0 + b;
    const int Np = a.nt * GP_TS, G = a.G;
    pair_mfma_body_sides<FREG, false, 0>(
        a, s, G, sm, a.m, a.mt * GP_TS, [&](int F, int g0, double* fr) { stage_scaled_features<GP_TS>(a, s, F, F, g0, fr); },
        [&](int F, int FS, int c0, double* fc) { stage_scaled_new_features<PM_CC>(a, s, F, FS, c0, fc); },
        [&](int i, int g, double, const double*) { return a.W[(long long)i * G + g]; },
        [&](int gj, int g0, int ng, const d4* acc, const d4*) {
            const bool in = gj < a.n;
            pair_mfma_each_column(ng, [&](int q, int v, int ll) { a.bw[(b * G + (g0 + ll)) * Np + gj] = in ? acc[q][v] : 0.0; });
        });
}

// part[ti, g] = sum_{i in row block ti} W[i, g] (B** W)[i, g]: new individuals on both sides, and the product is reduced against
// W before it leaves the workgroup — no m x G buffer.  Order of a column's sum, fixed: per wave and 16-row sub-tile the xor tree
// over the 16 rows (1, 2, 4, 8), sub-tile 0 + sub-tile 1, then the waves as (w0 + w1) + (w2 + w3).  Rows i >= m contribute 0.0.
// LDS: the body's layout, then red [4 waves][PM_NL].
constexpr int new_wsum_self_lds_bytes(int F, int FS) { return pair_mfma_lds_bytes(F, FS, false) + 4 * PM_NL * 8; }

template <int FREG>
__global__ __launch_bounds__(256, 2) void new_wsum_self_kernel(NewWsumArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const long long b = blockIdx.y, s = a.s0 + b;
    const int G = a.G, F = a.nU + a.nX;
    double* red = sm + pair_mfma_lds_bytes(F, FREG > F ? FREG : F, false) / 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double p[4][4];
    pair_mfma_body_sides<FREG, false, 0>(
        a, s, G, sm, a.m, a.mt * GP_TS, [&](int F_, int g0, double* fr) { stage_scaled_new_features<GP_TS>(a, s, F_, F_, g0, fr); },
        [&](int F_, int FS, int c0, double* fc) { stage_scaled_new_features<PM_CC>(a, s, F_, FS, c0, fc); },
        [&](int i, int g, double, const double*) { return a.W[(long long)i * G + g]; },
        [&](int gi, int g0, int ng, const d4* acc, const d4*) {
            const bool second = (gi >> 4) & 1;      // the body's sub-tile index (row = 128 ib + 32 wave + 16 sub + li): workgroup-uniform
            const double* wrow = a.W + (long long)gi * G + g0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int ll = 16 * q + (lane >> 4) + 4 * v;
                    const double t = (gi < a.m && ll < ng) ? wrow[ll] * acc[q][v] : 0.0;
                    p[q][v] = second ? p[q][v] + t : t;
                }
            if (!second) return;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    double x = p[q][v];
#pragma unroll
                    for (int o = 1; o <= 8; o <<= 1) x += __shfl_xor(x, o, 64);
                    if ((lane & 15) == 0) red[wave * PM_NL + 16 * q + (lane >> 4) + 4 * v] = x;
                }
            __syncthreads();
            // red is next written after the barriers of the next pass's chunk loop
            if (tid < ng)
                a.part[(b * a.mt + blockIdx.x) * G + g0 + tid] =
                    (red[tid] + red[PM_NL + tid]) + (red[2 * PM_NL + tid] + red[3 * PM_NL + tid]);
        });
}

// per (weight column, sample): beta_g = the row blocks' shares in ascending order, wnorm2_g = w_g . w_g (rhs_w_prepare_kernel's
// strided sum and tree), sumdelta[l + L g] = prior_l beta_g, and beta into slot 0 of the curve's prior (kappa, slot 1: 0.0)
template <int FORM>
__global__ __launch_bounds__(256) void new_wsum_finish_kernel(NewWsumArgs a) {
    __shared__ double red[4];
    __shared__ double s_beta;
    const int tid = threadIdx.x, g = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int G = a.G, L = a.lv.L;
    double ww = 0.0;
    for (int i = tid; i < a.m; i += 256) {
        const double w = a.W[(long long)i * G + g];
        ww = fma(w, w, ww);
    }
    const double w2 = block_sum_256(ww, red);
    if (tid == 0) {
        double beta = 0.0;
        for (int ti = 0; ti < a.mt; ++ti) beta += a.part[(b * a.mt + ti) * G + g];
        s_beta = beta;
        a.wnorm2[b * G + g] = w2;
        if (a.prior) {
            double* pr = a.prior + (b * G + g) * (L + 2);
            pr[0] = beta; pr[1] = 0.0;
        }
    }
    __syncthreads();
    const double beta = s_beta;
    for (int l = tid; l < L; l += 256) a.sumdelta[b * L * G + l + (long long)L * g] = new_prior<FORM>(a, s, l) * beta;
}

// ---------------------------------------------------------------------------------------
// Per-individual levels: mean[i, s, l] = sum_j B*_ij cross_ij(l) alpha_j with cross_ij from the ROW's dose a_il
// (and b_il) and the column's T_j.  cross no longer factors into a per-column term, so the product (B* R) of new_mean_mfma_kernel
// does not apply: a pass over the pairs in the shape of vec_pair_kernel<LB, false> (k_vec.hip).  One workgroup per (block of 128
// new individuals, block of LB levels, sample); thread (o = tid & 127, half = tid >> 7) owns new individual o and visits half of
// the 128 training individuals of every staged tile; the feature distance of a pair is evaluated once per level block, then one
// table-driven exp per level (two for the contrast).  Order of a sum, fixed: per thread along its columns in ascending column
// block, then half 0 + half 1.  A contrast with a_il == b_il is stored as 0.0.  New individuals that copy training rows, with the
// outcome form, run vec_pair_kernel's arithmetic for those rows.
// LDS (doubles): etab [32] | fo [F][128] new individuals | fk [F][128] training | tk [128] | ak [128] alpha | red [LB][128]
// ---------------------------------------------------------------------------------------
constexpr int new_mean_vec_lds_bytes(int F, int LB) { return (GP_EXP_TAB_DOUBLES + 2 * F * GP_TS + 2 * GP_TS + LB * GP_TS) * 8; }

template <int LB, int FORM>
__global__ __launch_bounds__(256) void new_mean_vec_kernel(NewArgs a) {
    using LF = LevelForm<FORM>;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int F = a.nU + a.nX;
    double* etab = sm;
    double* fo = etab + GP_EXP_TAB_DOUBLES;
    double* fk = fo + F * GP_TS;
    double* tk = fk + F * GP_TS;
    double* ak = tk + GP_TS;
    double* red = ak + GP_TS;
    const int tid = threadIdx.x, o = tid & 127, half = tid >> 7;
    const int ot = blockIdx.x, l0 = blockIdx.y * LB;
    const long long b = blockIdx.z, s = a.s0 + b;
    const int n = a.n, L = a.lv.L;
    const int go = ot * GP_TS + o;
    const bool own_in = go < a.m;

    stage_scaled_new_features<GP_TS>(a, s, F, F, ot * GP_TS, fo);
    gp_exp_tab_stage(etab, tid);

    const double ys = a.p.yScale[s];
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    double da[LB], db[LB];     // own doses per level (levels beyond L repeat the last one; their results are not written)
#pragma unroll
    for (int ll = 0; ll < LB; ++ll) {
        const long long at = go + (long long)a.m * min(l0 + ll, L - 1);
        da[ll] = own_in ? a.lv.doT[at] : 0.0;
        db[ll] = (LF::paired && own_in) ? a.lv.base[at] : 0.0;
    }
    double acc[LB];
#pragma unroll
    for (int ll = 0; ll < LB; ++ll) acc[ll] = 0.0;
    const double* alpha = a.alpha + b * (long long)a.nt * GP_TS;

    for (int kt = 0; kt < a.nt; ++kt) {
        const int k0 = kt * GP_TS;
        __syncthreads();
        stage_scaled_features<GP_TS>(a, s, F, F, k0, fk);
        if (tid < GP_TS) {
            tk[tid] = k0 + tid < n ? a.T[k0 + tid] : 0.0;
            ak[tid] = k0 + tid < n ? alpha[k0 + tid] : 0.0;
        }
        __syncthreads();
        // this half's columns of the tile: [64 half, 64 half + 64) below n (uniform per wave)
        const int rend = min(64, n - k0 - 64 * half);
#pragma unroll 1
        for (int rr = 0; rr < rend; ++rr) {
            const int r = 64 * half + rr;
            double lux = 0.0;
            for (int f = 0; f < F; ++f) {
                const double d = fo[f * GP_TS + o] - fk[f * GP_TS + r];
                lux = fma(d, d, lux);
            }
            const double Bv = ys * gp_exp_neg_tab(-lux, etab);
            const double tr = tk[r], al = ak[r];
#pragma unroll
            for (int ll = 0; ll < LB; ++ll) {
                const double dt = tr - da[ll], dbt = tr - db[ll];
                const double rb = LF::paired ? gp_exp_neg_tab(-((dbt * dbt) * wt), etab) : 0.0;
                acc[ll] = fma(Bv, LF::cross(dt, gp_exp_neg_tab(-((dt * dt) * wt), etab), rb, wt) * al, acc[ll]);
            }
        }
    }
    __syncthreads();
    if (half == 1) {
#pragma unroll
        for (int ll = 0; ll < LB; ++ll) red[ll * GP_TS + o] = acc[ll];
    }
    __syncthreads();
    if (half == 1 || !own_in) return;
    const int nl = min(LB, L - l0);
#pragma unroll
    for (int ll = 0; ll < LB; ++ll)
        if (ll < nl)
            a.mean[go + (long long)a.m * (s + a.S * (l0 + ll))] =
                (LF::paired && LF::zero_level(da[ll], db[ll])) ? 0.0 : acc[ll] + red[ll * GP_TS + o];
}

template <int LB, int FORM>
void launch_new_mean_vec_t(const NewArgs& a, int nbatch, hipStream_t st) {
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)new_mean_vec_kernel<LB, FORM>, new_mean_vec_lds_bytes(MAXF, LB));
    hipLaunchKernelGGL((new_mean_vec_kernel<LB, FORM>), dim3(a.mt, (a.lv.L + LB - 1) / LB, nbatch), dim3(256),
                       new_mean_vec_lds_bytes(a.nU + a.nX, LB), st, a);
}

// ---------------------------------------------------------------------------------------
// The test-set score (gpslc_y_test) on top of the outcome form at the test set's own treatments: C = B** o P -
// W* W*^T + yNoise I stands in the pair's Cm (mt + 1 tile rows, the identity on the padded diagonal) after minus_w_wt.
// ---------------------------------------------------------------------------------------
// the augmented row's tiles (mt, q): right-hand side 0 = Ytest - mean in row 0, zero on the padding; rows 1 .. 31 zero (the strip
// kernels handle a short augmented row in 32-row units), the other 96 have no reader.  One workgroup per (tile column, pair).
__global__ __launch_bounds__(256) void new_score_rhs_kernel(NewArgs a) {
    const int q = blockIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    double* __restrict__ aug = tref_tile(a.Cm, b, a.mt, q);
    const double* mean = a.mean + (long long)a.m * s;
    for (int idx = threadIdx.x; idx < GP_TS * 32; idx += 256) {
        const int c = idx >> 5, r = idx & 31, gi = GP_TS * q + c;
        aug[c * GP_TS + r] = (r == 0 && gi < a.m) ? a.Ytest[gi] - mean[gi] : 0.0;
    }
}

// lpd_i = log N(Ytest_i; mean_i, var_i); lpd_joint = -(m/2) log(2 pi) - log det(C)/2 - (Ytest - mean)^T C^-1 (Ytest - mean)/2, NaN
// where the factorisation of C broke down.  One workgroup per (row tile, pair).
__global__ __launch_bounds__(GP_TS) void new_score_finish_kernel(NewArgs a, int nbatch) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const long long b = blockIdx.y, s = a.s0 + b;
    const int gi = GP_TS * i + tid;
    if (a.lpd && gi < a.m) {
        const long long o = gi + (long long)a.m * s;
        const double v = a.var[o], r = a.Ytest[gi] - a.mean[o];
        a.lpd[o] = -0.91893853320467274178 - 0.5 * log(v) - 0.5 * ((r * r) / v);
    }
    if (i == 0 && tid == 0 && a.lpd_joint)
        a.lpd_joint[s] = a.pinfo[b] == 0 ? -0.91893853320467274178 * a.m - 0.5 * a.ldq[b] - 0.5 * a.ldq[nbatch + b] : NAN;
}

// the level forms new individuals can be asked for: the non-factual ones of level_form.h (run_predict refuses the others)
template <typename F>
void dispatch_new_form(int form, F&& f) {
    dispatch_form(form, [&](auto fm) {
        if constexpr (LevelForm<decltype(fm)::value>::factual) throw std::logic_error("new individuals have no factual treatment");
        else f(fm);
    });
}

// ... and those with per-individual levels: the outcome and the contrast
template <typename F>
void dispatch_new_vec_form(int form, F&& f) {
    if (form == FORM_OUTCOME) f(std::integral_constant<int, FORM_OUTCOME>{});
    else if (form == FORM_CONTRAST) f(std::integral_constant<int, FORM_CONTRAST>{});
    else throw std::logic_error("this level form has no per-individual levels for new individuals");     // run_predict refuses the call
}

}  // namespace

void launch_new_wsum(const NewWsumArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    const int F = a.nU + a.nX;
    pair_mfma_freg_ladder(F, [&](auto freg) {
        constexpr int FREG = decltype(freg)::value;
        pair_mfma_launch<new_wsum_cross_kernel<FREG>, FREG, false>(a, nbatch, st);
        static DeviceOnce attr_set;
        lds_opt_in(attr_set, (const void*)new_wsum_self_kernel<FREG>, new_wsum_self_lds_bytes(MAXF, MAXF));
        hipLaunchKernelGGL((new_wsum_self_kernel<FREG>), dim3(a.mt, nbatch), dim3(256),
                           new_wsum_self_lds_bytes(F, FREG > F ? FREG : F), st, a);
    });
    dispatch_new_form(a.lv.form, [&](auto form) {
        hipLaunchKernelGGL((new_wsum_finish_kernel<decltype(form)::value>), dim3(a.G, nbatch), dim3(256), 0, st, a);
    });
}

void launch_new_mean(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    dispatch_new_form(a.lv.form, [&](auto form) { launch_new_mean_t<decltype(form)::value>(a, nbatch, st); });
}
void launch_new_mean_vec(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    dispatch_new_vec_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        if (a.lv.L <= 1) launch_new_mean_vec_t<1, FORM>(a, nbatch, st);
        else if (a.lv.L <= 4) launch_new_mean_vec_t<4, FORM>(a, nbatch, st);
        else launch_new_mean_vec_t<8, FORM>(a, nbatch, st);
    });
}
void launch_new_score_rhs(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(new_score_rhs_kernel, dim3(a.mt, nbatch), dim3(256), 0, st, a);
}
void launch_new_score_finish(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(new_score_finish_kernel, dim3(a.mt, nbatch), dim3(GP_TS), 0, st, a, nbatch);
}
void launch_new_build(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    const int tiles = a.mt * a.nt + (a.Cm.base ? a.mt * (a.mt + 1) / 2 : 0);
    if (a.lv.vec) {
        dispatch_new_vec_form(a.lv.form, [&](auto form) {
            constexpr int FORM = decltype(form)::value;
            static DeviceOnce attr_set;
            lds_opt_in(attr_set, (const void*)new_build_kernel<FORM, true>, new_build_lds_bytes(MAXF, true));
            hipLaunchKernelGGL((new_build_kernel<FORM, true>), dim3(tiles, nbatch), dim3(256), new_build_lds_bytes(a.nU + a.nX, true), st, a);
        });
        return;
    }
    dispatch_new_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        static DeviceOnce attr_set;
        lds_opt_in(attr_set, (const void*)new_build_kernel<FORM, false>, new_build_lds_bytes(MAXF));
        hipLaunchKernelGGL((new_build_kernel<FORM, false>), dim3(tiles, nbatch), dim3(256), new_build_lds_bytes(a.nU + a.nX), st, a);
    });
}
void launch_new_var(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    if (a.lv.vec) {
        dispatch_new_vec_form(a.lv.form, [&](auto form) {
            hipLaunchKernelGGL((new_var_kernel<decltype(form)::value, true>), dim3(a.mt, nbatch), dim3(256), 0, st, a);
        });
        return;
    }
    dispatch_new_form(a.lv.form, [&](auto form) {
        hipLaunchKernelGGL((new_var_kernel<decltype(form)::value, false>), dim3(a.mt, nbatch), dim3(256), 0, st, a);
    });
}
void launch_new_gather(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(new_gather_kernel, dim3(a.mt * (a.mt + 1) / 2, nbatch), dim3(256), 0, st, a);
}
