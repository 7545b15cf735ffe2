// The level forms of a prediction call: what multiplies B_ij outside the pair loops.  Every kernel that knows about
// levels takes its per-form factors from LevelForm<FORM>; this is the one place the table is written.  With a = doT[l],
// b = doT_base[l], wt = 1 / tyLS^2, r^x_j = rho(T_j, x), rho(x, y) = exp(-(x - y)^2 wt): the callers evaluate the exponentials their
// own way (gp_rho, the table-driven exp, fp32) and hand the values over, and the operation order of every expression here is part
// of the results.  Needs <type_traits> and the includer's __host__ / __device__ only (tests/c/level_form_test.cpp: the CPU check).
// A fifth form takes one LevelForm specialisation, one line in dispatch_form, one row in kFormRules (predict.h) and one entry point.
#pragma once
#include <type_traits>

enum { FORM_ORDINARY = 0, FORM_CONTRAST = 1, FORM_SLOPE = 2, FORM_OUTCOME = 3 };   // f_i(a) - f_i(T_i), f_i(a) - f_i(b), d f_i / dt at a, f_i(a)

// q^a_j of the slope form: the difference dt = T_j - a is formed in fp64 by the caller's arguments
__host__ __device__ inline double gp_slope_q(double dt, double r, double wt) { return (2.0 * dt) * wt * r; }

//   factual         the estimand subtracts f_i(T_i): the - kw_j of the right-hand side, the - (Y_i - yNoise alpha_i) and the
//                   T_i == doT_l -> 0.0 rule of the mean, the e / g_ij terms of the tiles, kappa / gamma_l of the curve prior, and
//                   K W on the host.  That arithmetic is no product of one factor and stays in its kernel, behind this flag
//   paired          a second level doT_base[l] exists (r_b, rho_ab and the rho_.b' of joint are evaluated only then)
//   vector_levels, fp32_kernels   the kernels for per-individual levels / for GPSLC_FLAG_FP32_KERNEL exist for this form
//   cross(dt, r_a, r_b, wt)   the factor of B_ij, bw_j or alpha_j for column j, dt = T_j - a
//   prior(rho_ab, wt)         non-factual forms: Delta_ij = prior B_ij, so sum(Delta) = prior sum B and w' Delta w = prior w . bw
//   joint(rho_aa, rho_ab, rho_ba, rho_bb, d, wt)   the coefficient of beta = w . bw in P_ll' (k_curve.hip): rho_xy = rho(x_l, y_l'),
//                   d = a_l - a_l'.  joint of a level with itself is prior: the diagonal of covW is varW
//   zero_level(a, b)          the level's outputs are exact zeros whatever the data (a contrast of a level with itself)
template <int FORM> struct LevelForm;

template <> struct LevelForm<FORM_ORDINARY> {
    static constexpr bool factual = true, paired = false, vector_levels = true, fp32_kernels = true;
    __host__ __device__ static double cross(double, double r_a, double, double) { return r_a; }
    __host__ __device__ static double joint(double rho_aa, double, double, double, double, double) { return rho_aa; }
    __host__ __device__ static bool zero_level(double, double) { return false; }
};
template <> struct LevelForm<FORM_CONTRAST> {
    static constexpr bool factual = false, paired = true, vector_levels = false, fp32_kernels = false;
    __host__ __device__ static double cross(double, double r_a, double r_b, double) { return r_a - r_b; }
    __host__ __device__ static double prior(double rho_ab, double) { return (1.0 - rho_ab) + (1.0 - rho_ab); }
    __host__ __device__ static double joint(double rho_aa, double rho_ab, double rho_ba, double rho_bb, double, double) {
        return (rho_aa - rho_ab) - (rho_ba - rho_bb);
    }
    __host__ __device__ static bool zero_level(double a, double b) { return a == b; }
};
template <> struct LevelForm<FORM_SLOPE> {
    static constexpr bool factual = false, paired = false, vector_levels = false, fp32_kernels = false;
    __host__ __device__ static double cross(double dt, double r_a, double, double wt) { return gp_slope_q(dt, r_a, wt); }
    __host__ __device__ static double prior(double, double wt) { return 2.0 * wt; }
    __host__ __device__ static double joint(double rho_aa, double, double, double, double d, double wt) {
        return (2.0 * wt - 4.0 * (d * d) * (wt * wt)) * rho_aa;
    }
    __host__ __device__ static bool zero_level(double, double) { return false; }
};
template <> struct LevelForm<FORM_OUTCOME> {
    static constexpr bool factual = false, paired = false, vector_levels = true, fp32_kernels = false;
    __host__ __device__ static double cross(double, double r_a, double, double) { return r_a; }
    __host__ __device__ static double prior(double, double) { return 1.0; }
    __host__ __device__ static double joint(double rho_aa, double, double, double, double, double) { return rho_aa; }
    __host__ __device__ static bool zero_level(double, double) { return false; }
};

// Levels that depend on the (new) individual (outcome and contrast): individual i is set to a_i (against b_i).  The
// factor of B*_ij is cross with r_a = rho(T_j, a_i), r_b = rho(T_j, b_i), evaluated per pair; the factor of B**_ii' is joint between
// the levels of i and of i' — P_ii' below.  rho(x, y) is the caller's exponential.  P_ii equals prior(rho(a_i, b_i)) bit for bit
// ((1 - r) - (r - 1) and (1 - r) + (1 - r) round alike), and a contrast with a_i == b_i has P_ii' == 0.0 for every i'.
template <int FORM, class Rho>
__host__ __device__ inline double level_pair_prior(double ai, double bi, double aj, double bj, double wt, Rho&& rho) {
    using LF = LevelForm<FORM>;
    if constexpr (LF::paired) return LF::joint(rho(ai, aj), rho(ai, bj), rho(bi, aj), rho(bi, bj), ai - aj, wt);
    else return LF::joint(rho(ai, aj), 0.0, 0.0, 0.0, ai - aj, wt);
}

// run-time form -> template argument: f(std::integral_constant<int, FORM_*>{})
template <typename F>
inline void dispatch_form(int form, F&& f) {
    if (form == FORM_OUTCOME) f(std::integral_constant<int, FORM_OUTCOME>{});
    else if (form == FORM_SLOPE) f(std::integral_constant<int, FORM_SLOPE>{});
    else if (form == FORM_CONTRAST) f(std::integral_constant<int, FORM_CONTRAST>{});
    else f(std::integral_constant<int, FORM_ORDINARY>{});
}
