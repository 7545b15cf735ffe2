// Gradient of the outcome log-likelihood log N(Y; 0, A), A = K + yNoise I, K_ij = yScale exp(-sum_f ((w_if - w_jf) / ls_f)^2)
// over the features w = [U | X | T], ls = [uyLS; xyLS; tyLS] (Rasmussen & Williams §5.4.1).  With
// alpha = A^-1 Y, Q = alpha alpha^T - A^-1, P = Q o K, c = diag(A^-1) and D_ijf = w_if - w_jf from the RAW features:
//     dLS_f   =  (1 / ls_f^3) sum_ij P_ij D_ijf^2
//     dU_if   = -(2 / ls_f^2) sum_j P_ij D_ijf                        (f < nU)
//     dyNoise =  (alpha . alpha - sum_i c_i) / 2
//     dyScale =  (alpha . Y - n - yNoise (alpha . alpha - sum_i c_i)) / (2 yScale)        [= sum_ij P_ij / (2 yScale)]
//     dY      = -alpha
// A^-1 = W W^T with W = L^-T, the packed triangle k_loo.hip's callers leave (loo_w_index).
//
// grad_pair_kernel: one work item = one lower tile (ti, tj), tj <= ti, of one matrix.  K loop: the 128 x 128 tile
// sum_{k = ti}^{nt - 1} W(ti, k) W(tj, k)^T of A^-1 on v_mfma_f64_16x16x4_f64 with tile_gemm_nt_kernel's slab staging, LDS
// layout and 4 x 4 accumulators per wave (tile_common.h); both operands come straight from the packed triangle, the K range is
// the item's own.  Epilogue, on the accumulators: the scaled features of the two row blocks and alpha go into the slab LDS, K_rc
// is evaluated again (gp_exp_neg), P_rc replaces the accumulator (zero for rows and columns >= n: the padding of A^-1 is the
// identity), then the raw features take the place of the scaled ones and every feature is reduced: sum P D^2 over the tile, and
// for f < nU the row sums of P D and, off the diagonal, the column sums with the opposite sign (tile (tj, ti) = the transpose).
// An off-diagonal tile counts twice in the lengthscale sums.  No atomics: every item owns its slots of the workspace.
// With alpha, the features and the off-diagonal of W exact zeros on the padding, and D_rr = 0 on its diagonal, every padded term
// of these sums is an exact zero even unmasked: the mask guards against padding of alpha or W that is not zero, nothing else.
//
// Summation orders, all fixed: an element of A^-1 is one MFMA chain over ascending k; a lane adds its 64 elements in the order
// (n, v, m), lanes by xor-shuffle trees, waves as (w0 + w1) + (w2 + w3) or the two halves of a row / column in index order;
// grad_finish_kernel adds the tiles in ascending tile order.  Nothing depends on the chunk, the stream, the grid or the schedule
// that produced the factor.
#include "gpslc_internal.h"
#include "gp_math.h"
#include "tile_common.h"

// doubles of the epilogue's LDS image: two blocks of F feature rows, alpha of both blocks (first phase), the per-wave lengthscale
// sums and the halves of a feature's row and column sums
#define GRAD_FEAT(F) (2 * (F) * GP_TS)
#define GRAD_LDS_DOUBLES(F) (GRAD_FEAT(F) + 2 * GP_TS + 4 * (F) + 4 * GP_TS)
static size_t grad_lds_bytes(int F) { return std::max<size_t>(GEMM_LDS_BYTES, (size_t)GRAD_LDS_DOUBLES(F) * sizeof(double)); }

// One workgroup per CU: beside the 128 accumulator registers the epilogue (64 exp chains, the shuffle trees) takes the allocation
// to about 470 registers; bounded to 256 (two workgroups per CU, as tile_gemm_nt_kernel runs) it spills 195 of them.
__global__ __launch_bounds__(256) void grad_pair_kernel(GradArgs a, int nlow, int nbatch) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave & 1, wc = wave >> 1;
    const int li = lane & 15, lg = lane >> 4;
    double* lA = smem;                       // [2][KS][LROW]
    double* lB = smem + 2 * OPER_LDS;        // [2][KS][LROW]
    const int frow_a = lg * LROW + wr * 64 + li;
    const int frow_b = lg * LROW + wc * 64 + li;
    int loff[4];
    stage_offsets(tid, loff);
    const int F = a.F(), nU = a.nU, nt = a.nt;

    ticket_loop(a, (long long)nlow * nbatch, tid, [&](const long long item) {
        const int b = (int)(item / nlow);
        const int t = (int)(item - (long long)b * nlow);
        int ti, tj;
        tri_decode(t, ti, tj);
        const long long s = a.s0 + b;
        const double* __restrict__ Wb = a.W + (long long)b * a.w_bstride;
        const double* __restrict__ rowA = Wb + loo_w_index(nt, ti, ti) * (long long)GP_TSQ;     // W(ti, ti), W(ti, ti + 1), ..
        const double* __restrict__ rowB = Wb + loo_w_index(nt, tj, ti) * (long long)GP_TSQ;     // W(tj, ti), W(tj, ti + 1), ..
        const int nslab = (nt - ti) * (GP_TS / KS);

        // ---- acc[m][n][v] = [A^-1][ti 128 + wr 64 + 16 m + li][tj 128 + wc 64 + 16 n + lg + 4 v]
        d4 acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (d4){0.0, 0.0, 0.0, 0.0};
        {
            d2 ra[4], rb[4];     // staging set A
            d2 ra2[4], rb2[4];   // staging set B: loads run two slabs ahead of the MFMAs
            auto gload = [&](int sl, d2 (&xa)[4], d2 (&xb)[4]) {
                const long long so = (long long)sl * (KS * GP_TS);      // the tiles of a row are one contiguous run in ascending k
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xa[u] = *reinterpret_cast<const d2*>(rowA + so + (tid + 256 * u) * 2);
                    xb[u] = *reinterpret_cast<const d2*>(rowB + so + (tid + 256 * u) * 2);
                }
            };
            auto lstore = [&](int buf, const d2 (&xa)[4], const d2 (&xb)[4]) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    *reinterpret_cast<d2*>(lA + buf * OPER_LDS + loff[u]) = xa[u];
                    *reinterpret_cast<d2*>(lB + buf * OPER_LDS + loff[u]) = xb[u];
                }
            };
            auto compute = [&](int buf) {
                const double* pa = lA + buf * OPER_LDS + frow_a;
                const double* pb = lB + buf * OPER_LDS + frow_b;
#pragma unroll
                for (int ks = 0; ks < KS / 4; ++ks) {
                    double af[4], bf[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) af[m] = pa[ks * 4 * LROW + 16 * m];
#pragma unroll
                    for (int n = 0; n < 4; ++n) bf[n] = pb[ks * 4 * LROW + 16 * n];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n) acc[m][n] = mfma_step<0>(bf[n], af[m], acc[m][n]);
                }
            };
            gload(0, ra, rb);
            lstore(0, ra, rb);
            gload(1, ra, rb);          // nslab is a multiple of 8
            __syncthreads();
            for (int sl = 0; sl < nslab; sl += 2) {
                if (sl + 2 < nslab) gload(sl + 2, ra2, rb2);
                MFMA_PRIO_UP;
                compute(0);
                MFMA_PRIO_DOWN;
                lstore(1, ra, rb);
                KLOOP_BARRIER;
                if (sl + 3 < nslab) gload(sl + 3, ra, rb);
                MFMA_PRIO_UP;
                compute(1);
                MFMA_PRIO_DOWN;
                if (sl + 2 < nslab) lstore(0, ra2, rb2);
                KLOOP_BARRIER;       // after the last slab: every wave is done with the slabs, the epilogue's image takes their place
            }
        }

        // ---- epilogue, phase 1: P = (alpha_r alpha_c - [A^-1]_rc) K_rc on the accumulators -------------------------------------
        double* fr = smem;                   // [F][128]: features of the rows (tile row ti), then of the columns (tile row tj)
        double* fc = smem + F * GP_TS;
        double* al_r = smem + GRAD_FEAT(F);
        double* al_c = al_r + GP_TS;
        double* s_ls = al_c + GP_TS;         // [F][4]: a wave's share of sum P D_f^2
        double* s_half = s_ls + 4 * F;       // [2][128] halves of the row sums (by wc), [2][128] of the column sums (by wr)
        const int g_r = ti * GP_TS, g_c = tj * GP_TS;
        // thread (blk, r) stages individual r of the row block (blk = 0) or the column block (1), feature by feature
        const int st_g = ((tid >> 7) ? g_c : g_r) + (tid & (GP_TS - 1));
        double* st_dst = smem + (tid >> 7) * (F * GP_TS) + (tid & (GP_TS - 1));
#pragma unroll 1
        for (int f = 0; f < F; ++f)      // x * (1 / ls): stage_scaled_features' product
            st_dst[f * GP_TS] = st_g < a.n ? a.raw_column(s, f)[st_g] * (1.0 / a.ls(s, f)) : 0.0;
        al_r[tid] = st_g < a.n ? a.alpha[(long long)b * nt * GP_TS + st_g] : 0.0;      // al_r, then al_c
        __syncthreads();
        {
            // the padding mask as factors of K (1 or 0 per row, yScale or 0 per column): a select around the exp chain becomes a branch
            // per element, and the accumulators then live across 64 joins
            const double ys = a.p.yScale[s];
            const int r0 = wr * 64 + li, c0 = wc * 64 + lg;
            double rmask[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) rmask[m] = g_r + r0 + 16 * m < a.n ? 1.0 : 0.0;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = c0 + 16 * n + 4 * v;
                    const double ysc = g_c + c < a.n ? ys : 0.0;
                    const double ac = al_c[c];
                    double d2s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
                    for (int f = 0; f < F; ++f) {
                        const double zc = fc[f * GP_TS + c];
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const double d = fr[f * GP_TS + r0 + 16 * m] - zc;
                            d2s[m] = fma(d, d, d2s[m]);
                        }
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const double k = (ysc * rmask[m]) * gp_exp_neg(-d2s[m]);
                        double p = (al_r[r0 + 16 * m] * ac - acc[m][n][v]) * k;
                        // P is wanted HERE: left to itself the compiler sinks the 64 exp chains below the barrier to their first use
                        // and keeps the 64 squared distances alive (and spilled) until then
                        asm volatile("" : "+v"(p));
                        acc[m][n][v] = p;
                    }
                }
        }
        __syncthreads();

        // ---- phase 2: the raw features, and per feature the sums of P D^2 and P D ------------------------------------------------
#pragma unroll 1
        for (int f = 0; f < F; ++f) st_dst[f * GP_TS] = st_g < a.n ? a.raw_column(s, f)[st_g] : 0.0;
        __syncthreads();
        const bool offdiag = ti != tj;
#pragma unroll 1
        for (int f = 0; f < F; ++f) {
            const bool is_u = f < nU;
            double wrow[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) wrow[m] = fr[f * GP_TS + wr * 64 + li + 16 * m];
            double sq = 0.0;
            double rs[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = wc * 64 + lg + 16 * n + 4 * v;
                    const double wcol = fc[f * GP_TS + c];
                    double cs = 0.0;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const double d = wrow[m] - wcol;
                        const double pd = acc[m][n][v] * d;
                        sq = fma(pd, d, sq);
                        rs[m] += pd;
                        cs += pd;
                    }
                    if (is_u && offdiag) {      // column sums: over the 16 lanes li of a group lg, then the two waves wr
#pragma unroll
                        for (int o = 1; o <= 8; o <<= 1) cs += __shfl_xor(cs, o, 64);
                        if (li == 0) s_half[2 * GP_TS + wr * GP_TS + c] = cs;
                    }
                }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
            if (lane == 0) s_ls[4 * f + wave] = sq;
            if (is_u) {                          // row sums: over the four lane groups lg, then the two waves wc
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    rs[m] += __shfl_xor(rs[m], 16, 64);
                    rs[m] += __shfl_xor(rs[m], 32, 64);
                    if (lg == 0) s_half[wc * GP_TS + wr * 64 + li + 16 * m] = rs[m];
                }
                __syncthreads();
                const int r = tid & (GP_TS - 1);
                if (tid < GP_TS) {
                    a.part_u[((((long long)b * nt + ti) * nt + tj) * nU + f) * GP_TS + r] = s_half[r] + s_half[GP_TS + r];
                } else if (offdiag) {            // D_cr = -D_rc
                    a.part_u[((((long long)b * nt + tj) * nt + ti) * nU + f) * GP_TS + r] = -(s_half[2 * GP_TS + r] + s_half[3 * GP_TS + r]);
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if (tid < F) {
            const double v = (s_ls[4 * tid] + s_ls[4 * tid + 1]) + (s_ls[4 * tid + 2] + s_ls[4 * tid + 3]);
            a.part_ls[((long long)b * nlow + t) * F + tid] = offdiag ? 2.0 * v : v;
        }
        // ticket_loop's barrier ends the item: the next one's first slab may then overwrite the image
    });
}

// Blocks x < nt: tile row x of dU (the tile columns in ascending order) and of dY.  Block nt: the lengthscale gradients (the
// lower tiles in ascending packed order) and the closed forms of dyScale and dyNoise, their three sums each as 256 strided
// partial sums in ascending row order and block_sum_256's tree.
__global__ __launch_bounds__(256) void grad_finish_kernel(GradArgs a, int nlow) {
    __shared__ double red[4];
    const int x = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nt = a.nt, nU = a.nU, nX = a.nX, F = a.F(), n = a.n;
    const long long s = a.s0 + b, Np = (long long)nt * GP_TS;
    const bool bad = a.info[s] != 0;
    if (x < nt) {
        if (a.dU && a.part_u) {
            for (int idx = tid; idx < nU * GP_TS; idx += 256) {
                const int f = idx >> 7, r = idx & (GP_TS - 1);
                const int i = x * GP_TS + r;
                if (i >= n) continue;
                double sum = 0.0;
                for (int tj = 0; tj < nt; ++tj) sum += a.part_u[((((long long)b * nt + x) * nt + tj) * nU + f) * GP_TS + r];
                const double l = a.ls(s, f);
                a.dU[i + (long long)n * (f + (long long)nU * s)] = bad ? NAN : -2.0 * sum / (l * l);
            }
        }
        if (a.dY && tid < GP_TS) {
            const int i = x * GP_TS + tid;
            if (i < n) a.dY[i + (long long)n * s] = bad ? NAN : -a.alpha[b * Np + i];
        }
        return;
    }
    if (a.part_ls && tid < F) {
        double sum = 0.0;
        for (int t = 0; t < nlow; ++t) sum += a.part_ls[((long long)b * nlow + t) * F + tid];
        const double l = a.ls(s, tid);
        const double g = bad ? NAN : sum / (l * l * l);
        if (tid < nU) { if (a.duyLS) a.duyLS[s * nU + tid] = g; }
        else if (tid < nU + nX) { if (a.dxyLS) a.dxyLS[s * nX + (tid - nU)] = g; }
        else if (a.dtyLS) a.dtyLS[s] = g;
    }
    if (a.dyScale || a.dyNoise) {       // uniform over the launch: the barriers below are met by every thread
        double aa = 0.0, sc = 0.0, ay = 0.0;
        for (int i = tid; i < n; i += 256) {
            const double al = a.alpha[b * Np + i];
            aa = fma(al, al, aa);
            sc += a.c[b * Np + i];
            ay = fma(al, a.Y[s * a.y_sstride + i], ay);
        }
        aa = block_sum_256(aa, red);
        sc = block_sum_256(sc, red);
        ay = block_sum_256(ay, red);
        if (tid == 0) {
            const double ys = a.p.yScale[s], yn = a.p.yNoise[s];
            const double tr = aa - sc;
            if (a.dyNoise) a.dyNoise[s] = bad ? NAN : 0.5 * tr;
            if (a.dyScale) a.dyScale[s] = bad ? NAN : (ay - (double)n - yn * tr) / (2.0 * ys);
        }
    }
}

void launch_grad_pairs(const GradArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0 || !a.part_ls) return;
    const int nlow = a.nt * (a.nt + 1) / 2;
    const long long work = (long long)nlow * nbatch;
    const int slots = device_cus();         // persistent: one workgroup per CU (the kernel's registers), never more than items
    const size_t bytes = grad_lds_bytes(a.F());
    static DeviceOnce once;
    lds_opt_in(once, (const void*)grad_pair_kernel, (int)grad_lds_bytes(MAXF + 1));
    hipLaunchKernelGGL(grad_pair_kernel, dim3((unsigned)(work < slots ? work : slots)), dim3(256), bytes, st, a, nlow, nbatch);
}
void launch_grad_finish(const GradArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0) return;
    hipLaunchKernelGGL(grad_finish_kernel, dim3(a.nt + 1, nbatch), dim3(256), 0, st, a, a.nt * (a.nt + 1) / 2);
}
