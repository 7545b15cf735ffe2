// Leave-one-out predictive checks of the outcome model Y ~ N(0, A), A = K + yNoise I = L L^T (DESIGN.md §18;
// Rasmussen & Williams §5.4.2).  With alpha = A^-1 Y and c_i = [A^-1]_ii:
//     looMean_i = Y_i - alpha_i / c_i,   looVar_i = 1 / c_i,   looLpd_i = -log(2 pi)/2 + log(c_i)/2 - alpha_i^2 / (2 c_i).
// c = diag(A^-1) = diag(L^-T L^-1) = the squared row norms of W = L^-T: a sum of squares, no cancellation.  W is upper
// block-triangular; its O(n^3/3) products run on the f64 matrix cores (loo_diagonal_kernel, k_tilegemm.hip: strip_item with
// the K range of tile row i starting at i).  Here: the diagonal tiles W(i, i) = inv(L_ii)^T that start every row's chain, the
// row norms, and the kernel that turns alpha, c, Y into the outputs.
// Summation order of c_r, fixed: per column parity h of the tiles (two halves of the workgroup) ascending k, inside a tile
// ascending column in four interleaved partial sums ((p0 + p1) + (p2 + p3)); c_r = half 0 + half 1.  Nothing depends on the
// chunk, the stream or the schedule that produced the factor.
#include "gpslc_internal.h"

// W(i, i)[r, c] = inv(L_ii)[c, r] for c >= r, zero below the diagonal (the inverse is lower triangular: only that part is read)
__global__ __launch_bounds__(256) void loo_init_kernel(LooArgs a) {
    const int i = blockIdx.x, b = blockIdx.y;
    const double* __restrict__ src = a.inv + (long long)b * a.inv_bstride + (long long)i * GP_TSQ;
    double* __restrict__ dst = a.W + (long long)b * a.w_bstride + loo_w_index(a.nt, i, i) * (long long)GP_TSQ;
    for (int e = threadIdx.x; e < GP_TSQ; e += 256) {
        const int r = e & (GP_TS - 1), c = e >> 7;          // element (r, c) of a tile at c * 128 + r
        dst[e] = c >= r ? src[r * GP_TS + c] : 0.0;
    }
}

__global__ __launch_bounds__(256) void loo_rownorm_kernel(LooArgs a) {
    __shared__ double s_half[GP_TS];
    const int i = blockIdx.x, b = blockIdx.y;
    const int r = threadIdx.x & (GP_TS - 1), h = threadIdx.x >> 7;
    const double* __restrict__ row = a.W + (long long)b * a.w_bstride + loo_w_index(a.nt, i, i) * (long long)GP_TSQ;
    double acc = 0.0;
    for (int k = i; k < a.nt; ++k) {
        const double* __restrict__ t = row + (long long)(k - i) * GP_TSQ + r;
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
    if (h == 0) a.c[(long long)b * a.nt * GP_TS + (long long)i * GP_TS + r] = acc + s_half[r];
}

__global__ __launch_bounds__(256) void loo_finish_kernel(LooArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.n) return;                                   // padding rows are never read
    const long long s = a.s0 + b, Np = (long long)a.nt * GP_TS;
    double mean = NAN, var = NAN, lpd = NAN;
    if (a.info[s] == 0) {
        const double c = a.c[b * Np + i], al = a.alpha[b * Np + i], y = a.Y[s * a.y_sstride + i];
        mean = y - al / c;
        var = 1.0 / c;
        lpd = -0.91893853320467274178 + 0.5 * log(c) - 0.5 * (al * al) / c;
    }
    const long long o = (long long)a.n * s + i;
    if (a.looMean) a.looMean[o] = mean;
    if (a.looVar) a.looVar[o] = var;
    if (a.looLpd) a.looLpd[o] = lpd;
}

void launch_loo_init(const LooArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(loo_init_kernel, dim3(a.nt, nbatch), dim3(256), 0, st, a);
}
void launch_loo_rownorm(const LooArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(loo_rownorm_kernel, dim3(a.nt, nbatch), dim3(256), 0, st, a);
}
void launch_loo_finish(const LooArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(loo_finish_kernel, dim3((a.n + 255) / 256, nbatch), dim3(256), 0, st, a);
}
