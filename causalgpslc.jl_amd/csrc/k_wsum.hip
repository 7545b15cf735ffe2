// Weighted column sums of B and K for group-weighted average effects.
//
//   BW[i, g] = sum_j B_ij W[j, g]        KW[i, g] = sum_j B_ij e_ij W[j, g]
//
// with B = yScale exp(Lu + Lx), e_ij = exp(-(T_i - T_j)^2 / tyLS^2), K = B .* e (B and K are symmetric: these are the
// weighted column sums; W = 1 gives the bsum / ksum of the Gram build).  One workgroup = one row block of 128 individuals of
// one posterior sample, all G weight columns in passes of 64, on the pair-product body this kernel shares with
// ite_mean_mfma_kernel (pair_mfma.h: how B_rc and e_rc are evaluated, the fixed summation order, KW == BW bit for bit when
// e == 1 everywhere, zero features and zero weights for the columns j >= n, and why the FREG rung that serves an F cannot
// change a bit).  This file supplies the two things the body asks of a caller:
//   - what is staged: X[j, g] = W[j, g] (W is g-fastest: consecutive threads read consecutive weight columns);
//   - the store: bw / kw are [b][G][Np], rows i >= n are written as 0.0.
// WK = false (contrasts and slopes: c needs no KW): no e, no second MFMA, kw is not written.  BIN: binary treatments, e is 1 or
// exp(-1/tyLS^2).
#include "pair_mfma.h"

template <int FREG, bool WK, int BIN>   // FREG > 0: this lane's two rows' features live in registers (F <= FREG); 0: read from LDS
__global__ __launch_bounds__(256, 2) void wsum_mfma_kernel(WsumArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const long long b = blockIdx.y;
    const int Np = a.nt * GP_TS, G = a.G;
    pair_mfma_body<FREG, WK, BIN>(
        a, a.s0 + b, G, sm, [&](int j, int g, double, const double*) { return a.W[(long long)j * G + g]; },
        [&](int gi, int g0, int ng, const d4* accB, const d4* accK) {
            const bool in = gi < a.n;
            pair_mfma_each_column(ng, [&](int q, int v, int ll) {
                const long long o = (b * G + (g0 + ll)) * Np + gi;
                a.bw[o] = in ? accB[q][v] : 0.0;
                if constexpr (WK) a.kw[o] = in ? accK[q][v] : 0.0;
            });
        });
}

template <bool WK, int BIN>
static void launch_wsum_f(const WsumArgs& a, int nbatch, hipStream_t st) {
    pair_mfma_freg_ladder(a.nU + a.nX, [&](auto freg) {
        constexpr int FREG = decltype(freg)::value;
        pair_mfma_launch<wsum_mfma_kernel<FREG, WK, BIN>, FREG, WK>(a, nbatch, st);
    });
}
void launch_wsum(const WsumArgs& a, int nbatch, hipStream_t st) {
    if (!a.with_k) launch_wsum_f<false, 0>(a, nbatch, st);
    else if (a.binary_t) launch_wsum_f<true, 1>(a, nbatch, st);
    else launch_wsum_f<true, 0>(a, nbatch, st);
}
