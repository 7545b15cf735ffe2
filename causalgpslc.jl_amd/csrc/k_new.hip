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
// Further down: weighted averages over the new individuals, which need none of these tiles.
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
constexpr int new_build_lds_bytes(int F) { return (GP_EXP_TAB_DOUBLES + 2 * F * GP_TS + GP_TS) * 8; }

template <int FORM>
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
    if (cross && tid < GP_TS) {
        const int g = gj0 + tid;
        double v = 0.0;
        if (g < a.n) {
            const double t = a.T[g], doT = a.lv.doT[l];
            v = LF::cross(t - doT, gp_rho(t, doT, wt), LF::paired ? gp_rho(t, a.lv.base[l], wt) : 0.0, wt);
        }
        xc[tid] = v;
    }
    const double prior = cross ? 0.0 : new_prior<FORM>(a, s, l);
    __syncthreads();
    const double ys = a.p.yScale[s];
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
        const double xj = cross ? xc[cq] : prior;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rp = ty + 16 * p;
            const int gi = gi0 + rp;
            double v = 0.0;
            if (gi < a.m && gj < ncol) {
                v = (ys * gp_exp_neg_tab(-lux[p], etab)) * xj;
                if (!cross && gi == gj) v += a.pred_noise;
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
template <int FORM>
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
    if (h == 0 && gi < a.m)
        a.var[gi + (long long)a.m * (s + a.S * l)] = (new_prior<FORM>(a, s, l) * a.p.yScale[s] - (acc + s_half[r])) + a.pred_noise;
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

// the level forms new individuals can be asked for: the non-factual ones of level_form.h (run_predict refuses the others)
template <typename F>
void dispatch_new_form(int form, F&& f) {
    dispatch_form(form, [&](auto fm) {
        if constexpr (LevelForm<decltype(fm)::value>::factual) throw std::logic_error("new individuals have no factual treatment");
        else f(fm);
    });
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
void launch_new_build(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    const int tiles = a.mt * a.nt + (a.Cm.base ? a.mt * (a.mt + 1) / 2 : 0);
    dispatch_new_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        static DeviceOnce attr_set;
        lds_opt_in(attr_set, (const void*)new_build_kernel<FORM>, new_build_lds_bytes(MAXF));
        hipLaunchKernelGGL((new_build_kernel<FORM>), dim3(tiles, nbatch), dim3(256), new_build_lds_bytes(a.nU + a.nX), st, a);
    });
}
void launch_new_var(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    dispatch_new_form(a.lv.form, [&](auto form) {
        hipLaunchKernelGGL((new_var_kernel<decltype(form)::value>), dim3(a.mt, nbatch), dim3(256), 0, st, a);
    });
}
void launch_new_gather(const NewArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(new_gather_kernel, dim3(a.mt * (a.mt + 1) / 2, nbatch), dim3(256), 0, st, a);
}
