// Leave-group-out predictive checks of the outcome model Y ~ N(0, A), A = K + yNoise I = L L^T (Rasmussen &
// Williams §5.4.2 in block form).  For a group I of m individuals, C = [A^-1]_II and alpha = A^-1 Y:
//     mean_I = Y_I - C^-1 alpha_I,   cov_I = C^-1,   lpd_I = -(m/2) log(2 pi) + log det(C)/2 - alpha_I^T C^-1 alpha_I / 2.
// A^-1 = W W^T with W = L^-T (k_loo.hip leaves it as a packed triangle of tiles), so C = W[I, :] W[I, :]^T: a Gram matrix of
// rows of W, a sum of products with no subtraction from a prior term.  One workgroup per (group, sample):
//   1. gather the group's rows of W slab by slab (KC columns x mp rows, mp = m rounded up to 16, the rows beyond m zero) into
//      LDS and accumulate the lower 16 x 16 blocks of C on v_mfma_f64_16x16x4_f64;
//   2. C = R R^T in LDS (column Cholesky, sized to m), V = R^-1 by forward substitution into the unused upper triangle;
//   3. z = V alpha_I, C^-1 alpha_I = V^T z, var_i = the squared norm of column i of V (a sum of squares), log det C = 2 sum
//      log R_kk, alpha_I^T C^-1 alpha_I = z . z.
// Summation orders, all fixed: an element of C is one MFMA chain over the columns of W, ascending tile k from the tile row of
// the group's first member, ascending column inside the tile (four columns per instruction); a row contributes zeros before
// its own tile row.  The factorisation, V, z and the outputs are plain loops in ascending index.  Nothing depends on the label
// number, on the other groups, on the chunk, the stream or the schedule that produced the factor.
#include "gpslc_internal.h"
#include "sm_blocks.h"           // sm_tri_block

#define LGO_THREADS 256
#define LGO_NE 8        // slab elements per thread at most: KC * mp <= 256 * LGO_NE
#define LGO_NQ 9        // 16 x 16 blocks of C per wave at most: 36 lower blocks at mp = 128, four waves

// columns per slab: a whole tile's 128, halved until the slab has at most 2048 elements (mp = 16: 128; 32: 64; 48, 64: 32;
// 80 .. 128: 16) — small groups, the common case, pay one barrier and one global round trip per tile
__host__ __device__ inline int lgo_kc(int mp) {
    int kc = GP_TS;
    while (kc * mp > LGO_THREADS * LGO_NE) kc >>= 1;
    return kc;
}
// doubles of the region that holds the two slabs [2][KC][mp + 2] during the gather and C [mp][mp + 1] afterwards
__host__ __device__ inline int lgo_region(int mp) {
    const int slabs = 2 * lgo_kc(mp) * (mp + 2), cm = mp * (mp + 1);
    return slabs > cm ? slabs : cm;
}
// LDS bytes of a group of mp padded members: the region, alpha_I, z, the diagonal of R, its logarithms, the member rows
static size_t lgo_lds_bytes(int mp) { return ((size_t)lgo_region(mp) + 4 * (size_t)mp) * sizeof(double) + (size_t)mp * sizeof(int); }

__global__ __launch_bounds__(LGO_THREADS) void lgo_group_kernel(LgoArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int g = a.gmap ? a.gmap[blockIdx.x] : (int)blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const long long s = a.s0 + b, Np = (long long)a.nt * GP_TS;
    const int o0 = a.offsets[g], m = a.offsets[g + 1] - o0;
    const int mp = (m + 15) & ~15, nbk = mp >> 4;
    const int KC = lgo_kc(mp), LDM = mp + 2, LD = mp + 1;
    double* Cm = smem;                                  // after the gather: C, then R below and V above the diagonal
    double* s_al = smem + lgo_region(mp);
    double* s_z = s_al + mp;
    double* s_r = s_z + mp;
    double* s_logr = s_r + mp;
    int* s_rows = (int*)(s_logr + mp);

    auto write_nan = [&]() {
        for (int j = tid; j < m; j += LGO_THREADS) {
            const long long o = (long long)a.n * s + a.members[o0 + j];
            if (a.lgoMean) a.lgoMean[o] = NAN;
            if (a.lgoVar) a.lgoVar[o] = NAN;
        }
        if (tid == 0 && a.lgoLpd) a.lgoLpd[(long long)a.G * s + g] = NAN;
    };
    if (a.info[s] != 0) { write_nan(); return; }        // a broken factor: uniform over the workgroup

    if (tid < mp) {
        const int row = tid < m ? a.members[o0 + tid] : -1;
        s_rows[tid] = row;
        s_al[tid] = row >= 0 ? a.alpha[b * Np + row] : 0.0;
    }
    __syncthreads();

    // ---- 1. C = W[I, :] W[I, :]^T ---------------------------------------------------------------------------------
    {
        const double* __restrict__ Wb = a.W + (long long)b * a.w_bstride;
        const int k0 = s_rows[0] >> 7;                  // rows ascend: the first member's tile row is the smallest
        const int spt = GP_TS / KC, nslab = (a.nt - k0) * spt;
        const int ne = KC * mp / LGO_THREADS;           // exact: KC and mp are multiples of 16
        int e_ti[LGO_NE], e_off[LGO_NE], e_lds[LGO_NE];
#pragma unroll
        for (int e = 0; e < LGO_NE; ++e) {
            const int idx = tid + LGO_THREADS * e;
            const int c = idx / mp, j = idx - c * mp;
            const int row = e < ne ? s_rows[j] : -1;
            e_ti[e] = row >= 0 ? (row >> 7) : 0x7fffffff;       // a padding row never starts
            e_off[e] = c * GP_TS + (row & (GP_TS - 1));
            e_lds[e] = c * LDM + j;
        }
        double v[LGO_NE];
        auto load_slab = [&](int sl) {
            const int k = k0 + sl / spt, c0 = (sl % spt) * KC;
#pragma unroll
            for (int e = 0; e < LGO_NE; ++e)
                v[e] = e_ti[e] <= k ? Wb[loo_w_index(a.nt, e_ti[e], k) * (long long)GP_TSQ + c0 * GP_TS + e_off[e]] : 0.0;
        };
        // this wave's blocks of C: the lower blocks in row-major order, dealt round-robin to the four waves
        const int npair = nbk * (nbk + 1) / 2;
        const int nq = wave < npair ? (npair - wave + 3) / 4 : 0;
        int aoff[LGO_NQ], boff[LGO_NQ];
        d4 acc[LGO_NQ];
#pragma unroll
        for (int q = 0; q < LGO_NQ; ++q) {
            int bi, p;
            sm_tri_block(wave + 4 * q, bi, p);          // block (bi, bj = p)
            aoff[q] = lg * LDM + 16 * bi + li;
            boff[q] = lg * LDM + 16 * p + li;
            acc[q] = (d4){0.0, 0.0, 0.0, 0.0};
        }
        load_slab(0);
        for (int sl = 0; sl < nslab; ++sl) {
            double* buf = smem + (sl & 1) * KC * LDM;
#pragma unroll
            for (int e = 0; e < LGO_NE; ++e)
                if (e < ne) buf[e_lds[e]] = v[e];
            __syncthreads();
            if (sl + 1 < nslab) load_slab(sl + 1);
            for (int cc = 0; cc < KC; cc += 4) {
                const double* bc = buf + cc * LDM;
#pragma unroll
                for (int q = 0; q < LGO_NQ; ++q)
                    if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(bc[aoff[q]], bc[boff[q]], acc[q], 0, 0, 0);
            }
        }
        __syncthreads();                                // the slabs are read: C takes their place
#pragma unroll
        for (int q = 0; q < LGO_NQ; ++q) {
            if (q < nq) {
                int bi, p;
                sm_tri_block(wave + 4 * q, bi, p);
#pragma unroll
                for (int u = 0; u < 4; ++u) Cm[16 * bi + lg + 4 * u + (16 * p + li) * LD] = acc[q][u];
            }
        }
        __syncthreads();
    }

    // ---- 2. C = R R^T, column by column; thread (i, h) updates the columns of parity h of row i -------------------------
    // The loops below run over a wave's whole index range with the per-lane condition as a select (a term that does not belong
    // to a lane is an exact zero, or its store is masked): the LDS loads of several iterations are then in flight together,
    // where a loop with per-lane bounds pays one LDS round trip per term.  What they read beyond their own triangle is finite
    // (R, or the last value of a diagonal element) or unused.
    const int i = tid & (GP_TS - 1), h = tid >> 7;
    const int cw = tid & 64;                            // first row / column of this wave's 64
    const int imax = min(m - 1, cw + 63);
    bool bad = false;
    for (int j = 0; j < m; ++j) {
        const double d = Cm[j + j * LD];
        if (!(d > 0.0)) { bad = true; break; }          // every thread reads the same word: uniform
        const double rjj = sqrt(d);
        if (h == 0 && i > j && i < m) Cm[i + j * LD] /= rjj;
        if (tid == j) { s_r[j] = rjj; s_logr[j] = log(rjj); }
        __syncthreads();
        if (i > j && i < m) {
            const double lij = Cm[i + j * LD];
            for (int k = j + 1 + h; k <= imax; k += 8) {      // four columns of this thread's parity per pass
                double lk[4], cv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kk = min(k + 2 * u, imax);
                    lk[u] = Cm[kk + j * LD];
                    cv[u] = Cm[i + kk * LD];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + 2 * u <= i) Cm[i + (k + 2 * u) * LD] = fma(-lij, lk[u], cv[u]);
            }
        }
        __syncthreads();
    }
    if (bad) { write_nan(); return; }

    // V = R^-1 (lower triangular), column c by thread c, kept transposed above the diagonal: V[k, c] at Cm[c + k LD], c < k;
    // V[c, c] = 1 / R_cc.  V[k, c] = -(sum_{q = c}^{k - 1} R[k, q] V[q, c]) / R_kk, q ascending.
    if (tid < m) {
        const int c = tid;
        const double vcc = 1.0 / s_r[c];
        for (int k = cw + 1; k < m; ++k) {
            double sum = 0.0;
#pragma unroll 4
            for (int q = cw; q < k; ++q) {
                const double vq = Cm[c + q * LD];
                sum = fma(Cm[k + q * LD], q > c ? vq : (q == c ? vcc : 0.0), sum);
            }
            if (k > c) Cm[c + k * LD] = -sum / s_r[k];
        }
    }
    __syncthreads();

    // ---- 3. z = V alpha_I; C^-1 alpha_I = V^T z; var = squared column norms of V ----------------------------------------
    if (tid < m) {
        const int k = tid;
        double z = 0.0;
#pragma unroll 4
        for (int c = 0; c < imax; ++c) {
            const double vkc = Cm[c + k * LD];
            z = fma(c < k ? vkc : 0.0, s_al[c], z);
        }
        s_z[k] = z + s_al[k] / s_r[k];
    }
    __syncthreads();
    if (tid < m) {
        const double vii = 1.0 / s_r[tid];
        double var = vii * vii, u = vii * s_z[tid];
#pragma unroll 4
        for (int k = cw + 1; k < m; ++k) {
            const double vki = Cm[tid + k * LD];
            const double w = k > tid ? vki : 0.0;
            var = fma(w, w, var);
            u = fma(w, s_z[k], u);
        }
        const int row = s_rows[tid];
        const long long o = (long long)a.n * s + row;
        if (a.lgoMean) a.lgoMean[o] = a.Y[s * a.y_sstride + row] - u;
        if (a.lgoVar) a.lgoVar[o] = var;
    }
    if (tid == 0 && a.lgoLpd) {
        double quad = 0.0, ld = 0.0;
        for (int k = 0; k < m; ++k) { quad = fma(s_z[k], s_z[k], quad); ld += s_logr[k]; }
        a.lgoLpd[(long long)a.G * s + g] = -0.91893853320467274178 * m + ld - 0.5 * quad;
    }
}

void launch_lgo_groups(const LgoArgs& a, int nbatch, hipStream_t st) {
    const int ng = a.gmap ? a.ngroups : a.G;        // a subset of the groups (gpslc_y_kfold's small ones), or all of them
    if (nbatch <= 0 || ng <= 0) return;
    // one launch covers groups of every size up to mmax: the LDS of the largest layout among them
    size_t bytes = 0;
    for (int mp = 16; mp <= ((a.mmax + 15) & ~15); mp += 16) bytes = std::max(bytes, lgo_lds_bytes(mp));
    static DeviceOnce once;
    lds_opt_in(once, (const void*)lgo_group_kernel, (int)lgo_lds_bytes(LGO_MAX_GROUP));
    hipLaunchKernelGGL(lgo_group_kernel, dim3(ng, nbatch), dim3(LGO_THREADS), bytes, st, a);
}
