// Per-individual intervention vectors ("vector levels", gpslc_predict_vec and friends).
//
// A vector level d (n values) replaces fill(doT, n) in src/likelihood.jl:27-28.  With B_ij = yScale exp(rbfKernelLog over
// U and X)_ij, e_ij = exp(-(T_i - T_j)^2 / tyLS^2), g_ij = exp(-(T_i - d_j)^2 / tyLS^2) and h_ij = exp(-(d_i - d_j)^2 / tyLS^2):
//     D = CovWWs' - CovWW,    D_ij = B_ij (g_ji - e_ij)
//     Delta_ij = B_ij ((e_ij - g_ij - g_ji) + h_ij)
// The scalar level's shortcuts (g_ji = r_j, h = 1: c = r .* bsum - ksum, sum(Delta) from column sums) do not apply: g and h
// are not separable, so the level's right-hand side c = D' 1, sum(Delta) and MeanITE = D alpha take a pass over the pairs
// per (sample, level).  The two kernels here are those passes; the factorisation, epilogue, back-substitution and unit B
// are shared with the scalar path (unit B's D / Delta tiles: dt_build_kernel<true>, k_solve.hip).
//
//   vec_pair_kernel<LB, true>   c_j = sum_i B_ij (g_ji - e_ij) into row 1 + l of the augmented right-hand-side tiles, and per tile of
//                     columns  sum_j [ sum_i B_ij (h_ij - e_ij) - 2 c_j ]  (= that tile's share of 1' Delta 1: the sums of
//                     B (g_ij - e_ij) and B (g_ji - e_ij) over all pairs are equal, B and e being symmetric)
//   vec_sumdelta_kernel   1' Delta 1 per (sample, level) from the per-tile shares, in tile order
//   vec_pair_kernel<LB, false>  MeanITE_i = sum_j B_ij g_ji alpha_j - (Y_i - yNoise alpha_i)   (K alpha = Y - yNoise alpha, as in
//                     ite_mean_kernel), and exactly 0.0 where d_i == T_i (row i of D is identically zero there)
//
// Both kernels: one workgroup per (tile of 128 "own" individuals, block of LB levels, sample); thread (o = tid & 127,
// half = tid >> 7) owns individual o and visits half of the 128 "other" individuals of every staged tile.  Every reduction
// has a fixed order (per thread along the others, then half 0 + half 1, then a fixed tree over the tile, then tile order),
// so results are bit-reproducible and do not depend on how the samples are chunked.  fp64 throughout.
// If d == T everywhere, g == e and h == e bit for bit (the same squares into the same exp), so c, Delta and MeanITE are
// exact zeros.
//
// FORM (VecArgs::lv.form) is one of the forms with vector levels (level_form.h): the ordinary form, all of the above, or one
// without a factual term — the potential outcome f_i(d_i) itself, the ordinary form with its factual terms dropped —
//     D_ij = B_ij g_ji,    Delta_ij = B_ij h_ij
//   sums   c_j = sum_i B_ij g_ji, and per tile of columns sum_j sum_i B_ij h_ij alone; no e is evaluated (two exps per pair
//          and level, as before)
//   mean   MeanITE_i = sum_j B_ij g_ji alpha_j: no K alpha term and no d_i == T_i rule
// in the same reduction orders.
#include "gpslc_internal.h"
#include "gp_math.h"
#include <stdexcept>

template <int LB, bool SUMS, int FORM>
__global__ __launch_bounds__(256) void vec_pair_kernel(VecArgs a) {
    constexpr bool FACTUAL = LevelForm<FORM>::factual;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int F = a.nU + a.nX;
    double* etab = sm;                          // [32] 2^(j/32): table-driven exp (gp_math.h)
    double* fo = etab + GP_EXP_TAB_DOUBLES;     // [F][128] own features / LS
    double* fk = fo + F * GP_TS;                // [F][128] other features / LS
    double* tk = fk + F * GP_TS;                // [128] T of the others
    double* xk = tk + GP_TS;                    // SUMS: [LB][128] d of the others;  mean: [128] alpha of the others
    double* red = xk + LB * GP_TS;              // [2][LB][128] half 1's accumulators
    const int tid = threadIdx.x, o = tid & 127, half = tid >> 7;
    const int ot = blockIdx.x, l0 = blockIdx.y * LB;
    const long long b = blockIdx.z, s = a.s0 + b;
    const int n = a.n;
    const int go = ot * GP_TS + o;
    const bool own_in = go < n;

    stage_scaled_features<GP_TS>(a, s, F, F, ot * GP_TS, fo);
    gp_exp_tab_stage(etab, tid);

    const double ys = a.p.yScale[s];
    const double tl = a.p.tyLS[s];
    const double wt = 1.0 / (tl * tl);
    const double to = own_in ? a.T[go] : 0.0;
    double dlo[LB];     // own d per level (levels beyond L repeat the last one; their results are not written)
#pragma unroll
    for (int ll = 0; ll < LB; ++ll) dlo[ll] = own_in ? a.lv.doT[go + (long long)n * min(l0 + ll, a.lv.L - 1)] : 0.0;
    double acc[LB], acc2[LB];
#pragma unroll
    for (int ll = 0; ll < LB; ++ll) { acc[ll] = 0.0; acc2[ll] = 0.0; }
    const double* alpha = SUMS ? nullptr : a.alpha + b * (long long)a.nt * GP_TS;

    for (int kt = 0; kt < a.nt; ++kt) {
        const int k0 = kt * GP_TS;
        __syncthreads();
        stage_scaled_features<GP_TS>(a, s, F, F, k0, fk);
        if (tid < GP_TS) tk[tid] = k0 + tid < n ? a.T[k0 + tid] : 0.0;
        if (SUMS) {
            for (int idx = tid; idx < LB * GP_TS; idx += 256) {
                const int ll = idx >> 7, r = idx & 127;
                xk[idx] = k0 + r < n ? a.lv.doT[k0 + r + (long long)n * min(l0 + ll, a.lv.L - 1)] : 0.0;
            }
        } else if (tid < GP_TS) {
            xk[tid] = k0 + tid < n ? alpha[k0 + tid] : 0.0;
        }
        __syncthreads();
        // this half's others of the tile: [64 half, 64 half + 64) below n (uniform per wave)
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
            const double tr = tk[r];
            if (SUMS && !FACTUAL) {
#pragma unroll
                for (int ll = 0; ll < LB; ++ll) {
                    const double dk = xk[ll * GP_TS + r];
                    const double dg = to - dk, dh = dlo[ll] - dk;
                    acc[ll] = fma(Bv, gp_exp_neg_tab(-((dg * dg) * wt), etab), acc[ll]);      // g_{own,other}: T_own - d_other
                    acc2[ll] = fma(Bv, gp_exp_neg_tab(-((dh * dh) * wt), etab), acc2[ll]);
                }
            } else if (SUMS) {
                const double de = to - tr;
                const double Ev = gp_exp_neg_tab(-((de * de) * wt), etab);
#pragma unroll
                for (int ll = 0; ll < LB; ++ll) {
                    const double dk = xk[ll * GP_TS + r];
                    const double dg = to - dk, dh = dlo[ll] - dk;
                    const double Gv = gp_exp_neg_tab(-((dg * dg) * wt), etab);     // g_{own,other}: T_own - d_other
                    const double Hv = gp_exp_neg_tab(-((dh * dh) * wt), etab);
                    acc[ll] = fma(Bv, Gv - Ev, acc[ll]);
                    acc2[ll] = fma(Bv, Hv - Ev, acc2[ll]);
                }
            } else {
                const double ak = xk[r];
#pragma unroll
                for (int ll = 0; ll < LB; ++ll) {
                    const double dg = tr - dlo[ll];                                  // g_{other,own}: T_other - d_own
                    acc[ll] = fma(Bv, gp_exp_neg_tab(-((dg * dg) * wt), etab) * ak, acc[ll]);
                }
            }
        }
    }
    __syncthreads();
    if (half == 1) {
#pragma unroll
        for (int ll = 0; ll < LB; ++ll) {
            red[ll * GP_TS + o] = acc[ll];
            if (SUMS) red[(LB + ll) * GP_TS + o] = acc2[ll];
        }
    }
    __syncthreads();
    const int nl = min(LB, a.lv.L - l0);
    if (!SUMS) {
        if (half == 1 || !own_in) return;
        if (!FACTUAL) {
#pragma unroll
            for (int ll = 0; ll < LB; ++ll)
                if (ll < nl)
                    a.meanITE[(long long)go * a.si + s * a.ss + (long long)(l0 + ll) * a.sl] = acc[ll] + red[ll * GP_TS + o];
            return;
        }
        const double ka = a.Y[s * a.y_sstride + go] - a.p.yNoise[s] * alpha[go];      // (K alpha)_o: alpha solves (K + yNoise I) alpha = Y
#pragma unroll
        for (int ll = 0; ll < LB; ++ll)
            if (ll < nl) {
                const double v = (acc[ll] + red[ll * GP_TS + o]) - ka;
                a.meanITE[(long long)go * a.si + s * a.ss + (long long)(l0 + ll) * a.sl] = (dlo[ll] == to) ? 0.0 : v;
            }
        return;
    }
    // half 0 (waves 0 and 1): c_o into the augmented tiles, and the tile's share of 1' Delta 1 (fixed butterfly per wave,
    // then wave 0 + wave 1)
    __shared__ double wsum[2][LB];
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int ll = 0; ll < LB; ++ll) {
        double v = 0.0;
        if (half == 0) {
            const double c = acc[ll] + red[ll * GP_TS + o];
            const double hs = acc2[ll] + red[(LB + ll) * GP_TS + o];
            const int q = 1 + l0 + ll;
            if (own_in && ll < nl) tref_tile(a.M, b, a.nt + (q >> 7), ot)[o * GP_TS + (q & 127)] = c;
            if (own_in) v = FACTUAL ? hs - 2.0 * c : hs;
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
        if (lane == 0 && wave < 2) wsum[wave][ll] = v;
    }
    __syncthreads();
    if (tid < nl) a.part[((long long)b * a.lv.L + l0 + tid) * a.nt + ot] = wsum[0][tid] + wsum[1][tid];
}

// 1' Delta 1 of every (sample, level): the per-tile shares in tile order.  One workgroup per sample.
__global__ __launch_bounds__(256) void vec_sumdelta_kernel(VecArgs a) {
    const long long b = blockIdx.x;
    for (int l = threadIdx.x; l < a.lv.L; l += 256) {
        const double* p = a.part + ((long long)b * a.lv.L + l) * a.nt;
        double v = 0.0;
        for (int t = 0; t < a.nt; ++t) v += p[t];
        a.sumdelta[b * a.lv.L + l] = v;
    }
}

template <int LB, bool SUMS, int FORM>
static void launch_vec_t(const VecArgs& a, int nbatch, hipStream_t st) {
    const int F = a.nU + a.nX;
    const int bytes = (GP_EXP_TAB_DOUBLES + 2 * F * GP_TS + GP_TS + LB * GP_TS + 2 * LB * GP_TS) * 8;
    static DeviceOnce attr_set;
    lds_opt_in(attr_set, (const void*)vec_pair_kernel<LB, SUMS, FORM>,
               (GP_EXP_TAB_DOUBLES + 2 * MAXF * GP_TS + GP_TS + 3 * LB * GP_TS) * 8);
    hipLaunchKernelGGL((vec_pair_kernel<LB, SUMS, FORM>), dim3(a.nt, (a.lv.L + LB - 1) / LB, nbatch), dim3(256), bytes, st, a);
}
template <bool SUMS, int FORM>
static void launch_vec_f(const VecArgs& a, int nbatch, hipStream_t st) {
    if (a.lv.L <= 1) launch_vec_t<1, SUMS, FORM>(a, nbatch, st);
    else if (a.lv.L <= 4) launch_vec_t<4, SUMS, FORM>(a, nbatch, st);
    else launch_vec_t<8, SUMS, FORM>(a, nbatch, st);
}
template <bool SUMS>
static void launch_vec(const VecArgs& a, int nbatch, hipStream_t st) {
    dispatch_form(a.lv.form, [&](auto form) {
        constexpr int FORM = decltype(form)::value;
        if constexpr (LevelForm<FORM>::vector_levels) launch_vec_f<SUMS, FORM>(a, nbatch, st);
        else throw std::logic_error("this level form has no vector-level kernels");     // run_predict refuses the call
    });
}

void launch_vec_sums(const VecArgs& a, int nbatch, hipStream_t st) {
    launch_vec<true>(a, nbatch, st);
    hipLaunchKernelGGL(vec_sumdelta_kernel, dim3(nbatch), dim3(256), 0, st, a);
}
void launch_vec_mean(const VecArgs& a, int nbatch, hipStream_t st) { launch_vec<false>(a, nbatch, st); }
