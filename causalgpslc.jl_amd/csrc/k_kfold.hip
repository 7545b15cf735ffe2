// K-fold cross-validation of the outcome model: leave-group-out checks for groups of more than LGO_MAX_GROUP members
// (gpslc_y_kfold).  The mathematics is k_lgo.hip's: for a group I of m individuals, C = [A^-1]_II =
// W[I, :] W[I, :]^T with W = L^-T, and
//     mean_I = Y_I - C^-1 alpha_I,   var_I = diag(C^-1),   lpd_I = -(m/2) log(2 pi) + log det(C)/2 - alpha_I^T C^-1 alpha_I / 2.
// C no longer fits one workgroup's LDS, so it goes to HBM as an mt x mt triangle of 128 x 128 tiles, mt = ceil(m / 128), with
// alpha_I as its augmented row, and the factor layer that factorises A factorises it (factor_panels); the back-substitution gives
// C^-1 alpha_I, the epilogue log det C and the quadratic form, and §18's W = L_C^-T with its squared row norms diag(C^-1).  Here:
//   kfold_gram_kernel     one workgroup per (lower tile (p, q) of C, (group, sample) pair): gathers the member rows 128 p .. and
//                         128 q .. of the packed W slab by slab (KF_KC columns, two slabs in flight) into LDS and accumulates the
//                         tile on v_mfma_f64_16x16x4_f64, four waves of 4 x 4 accumulator blocks; the diagonal tiles' workgroups
//                         also write the augmented row;
//   kfold_finish_kernel   C^-1 alpha_I, diag(C^-1), log det C, the quadratic form -> cvMean, cvVar, cvLpd.
// Summation order of an element of C, fixed: one MFMA chain over the columns of W, ascending tile k, ascending column inside the
// tile (four columns per instruction).  A row contributes exact zeros before its own tile row, and the chain of tile (p, q) starts
// at the tile row of the first member of row block p: every row of either block is zero or absent before it, so the chain equals
// the one from the group's first tile row bit for bit (the skipped terms add +0.0 to +0.0).  Nothing depends on the label, on the
// other groups of the call, on the sub-batch or on the chunk.
// Padding (the convention of launch_dt_build / launch_new_build): rows beyond m are zero, the padded diagonal is the identity,
// the augmented row is zero there: the padded part of the factor is the identity and contributes log 1 = 0 and nothing else.
#include "gpslc_internal.h"

#define KF_THREADS 256
#define KF_KC 16                 // columns of W per slab
#define KF_LD (GP_TS + 16)       // doubles per slab column: the two k-rows a 32-lane half reads with ds_read_b64 are 288 dwords
                                 // apart, = 32 mod 64: disjoint halves of the 64-bank row (the padding of k_tilegemm.hip's slabs)
#define KF_SLAB (KF_KC * KF_LD)  // doubles of one operand's slab
#define KF_LDS_BYTES (2 * 2 * KF_SLAB * (int)sizeof(double))      // two slabs in flight x two operands: 73,728 bytes

// batch element b of a launch is pair p0 + b of its class: (sample (p0 + b) / ng of the chunk, group large[(p0 + b) % ng])
__device__ __forceinline__ void kfold_pair(const KfoldArgs& a, int b, int& sb, int& g) {
    const long long pr = a.p0 + b;
    sb = (int)(pr / a.ng);
    g = a.large[pr - (long long)sb * a.ng];
}

__global__ __launch_bounds__(KF_THREADS) void kfold_gram_kernel(KfoldArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    int p, q;
    tri_decode(blockIdx.x, p, q);                       // tile (p, q) of C, q <= p
    const int b = blockIdx.y;
    int sb, g;
    kfold_pair(a, b, sb, g);
    const int o0 = a.offsets[g], m = a.offsets[g + 1] - o0;
    const long long Np = (long long)a.nt * GP_TS;
    const bool diag = p == q;                           // uniform: one slab serves both operands

    // this thread's row of either block (j) and its columns of a slab (ch, ch + 2, ...)
    const int j = tid & (GP_TS - 1), ch = tid >> 7;
    const int jp = GP_TS * p + j, jq = GP_TS * q + j;
    const int rowP = jp < m ? a.members[o0 + jp] : -1, rowQ = jq < m ? a.members[o0 + jq] : -1;
    const int tiP = rowP >= 0 ? (rowP >> 7) : 0x7fffffff, tiQ = rowQ >= 0 ? (rowQ >> 7) : 0x7fffffff;      // a padding row never starts
    const int offP = rowP & (GP_TS - 1), offQ = rowQ & (GP_TS - 1);
    const int k0 = a.members[o0 + GP_TS * p] >> 7;      // rows ascend: every row of block p is zero before this tile row
    const double* __restrict__ Wb = a.W + (long long)sb * a.w_bstride;
    constexpr int spt = GP_TS / KF_KC, NE = KF_KC / 2;
    const int nslab = (a.nt - k0) * spt;

    double vP[NE], vQ[NE];
    auto load_slab = [&](int sl) {
        const int k = k0 + sl / spt, c0 = (sl % spt) * KF_KC + ch;
        const bool liveP = tiP <= k, liveQ = !diag && tiQ <= k;
        const double* tp = Wb + (liveP ? loo_w_index(a.nt, tiP, k) * (long long)GP_TSQ + offP : 0);
        const double* tq = Wb + (liveQ ? loo_w_index(a.nt, tiQ, k) * (long long)GP_TSQ + offQ : 0);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            vP[e] = liveP ? tp[(c0 + 2 * e) * GP_TS] : 0.0;
            vQ[e] = liveQ ? tq[(c0 + 2 * e) * GP_TS] : 0.0;
        }
    };

    // wave w: the 4 x 4 blocks of rows 64 (w >> 1) .. of block p against rows 64 (w & 1) .. of block q.  The MFMA's A operand is
    // the q side, its B operand the p side: lane & 15 then runs along the row index of the column-major output tile.
    const int rb = (wave >> 1) * 4, cb = (wave & 1) * 4;
    const int frow = lg * KF_LD + li;
    d4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] = (d4){0.0, 0.0, 0.0, 0.0};

    load_slab(0);
    for (int sl = 0; sl < nslab; ++sl) {
        double* bufP = smem + (sl & 1) * 2 * KF_SLAB;
        double* bufQ = diag ? bufP : bufP + KF_SLAB;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            bufP[(ch + 2 * e) * KF_LD + j] = vP[e];
            if (!diag) bufQ[(ch + 2 * e) * KF_LD + j] = vQ[e];
        }
        __syncthreads();                                // slab sl is whole; every wave is done with slab sl - 1
        if (sl + 1 < nslab) load_slab(sl + 1);
#pragma unroll
        for (int cc = 0; cc < KF_KC; cc += 4) {
            const double* rp = bufP + cc * KF_LD + frow + 16 * rb;
            const double* rq = bufQ + cc * KF_LD + frow + 16 * cb;
            double xp[4], xq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { xp[i] = rp[16 * i]; xq[i] = rq[16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xq[jj], xp[i], acc[i][jj], 0, 0, 0);
        }
    }

    // element (row r of block p, column c of block q) at c * 128 + r; accumulator u of a lane: c = lg + 4 u, r = li
    double* __restrict__ tile = tref_tile(a.Cm, b, p, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = 16 * (rb + i) + li;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 16 * (cb + jj) + lg + 4 * u;
                const bool unit = diag && r == c && GP_TS * p + r >= m;     // the padded diagonal
                tile[c * GP_TS + r] = unit ? 1.0 : acc[i][jj][u];
            }
        }
    }
    if (!diag) return;
    // the augmented row's tile (mt, q): right-hand side 0 = alpha_I in row 0, zero on the padding; the rows 1 .. 31 are zero (the
    // strip kernels handle a short augmented row in 32-row units, rhs_tiles_kernel), the other 96 have no reader
    double* __restrict__ aug = tref_tile(a.Cm, b, a.mt, q);
    const double* __restrict__ al = a.alpha + (long long)sb * Np;
    for (int idx = tid; idx < GP_TS * 32; idx += KF_THREADS) {
        const int c = idx >> 5, r = idx & 31, jc = GP_TS * q + c;
        aug[c * GP_TS + r] = (r == 0 && jc < m) ? al[a.members[o0 + jc]] : 0.0;
    }
}

// one workgroup per (tile row of C, pair): a sample whose factorisation of A broke down, or a pair whose factorisation of C did,
// gets NaN
__global__ __launch_bounds__(GP_TS) void kfold_finish_kernel(KfoldArgs a) {
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int sb, g;
    kfold_pair(a, b, sb, g);
    const int o0 = a.offsets[g], m = a.offsets[g + 1] - o0;
    const long long s = a.s0 + sb, Nc = (long long)a.mt * GP_TS;
    const bool ok = a.info[s] == 0 && a.pinfo[b] == 0;
    const int j = GP_TS * i + tid;
    if (j < m) {
        const int row = a.members[o0 + j];
        const long long o = (long long)a.n * s + row;
        if (a.cvMean) a.cvMean[o] = ok ? a.Y[s * a.y_sstride + row] - a.u[b * Nc + j] : NAN;
        if (a.cvVar) a.cvVar[o] = ok ? a.cdiag[b * Nc + j] : NAN;
    }
    if (i == 0 && tid == 0 && a.cvLpd)
        a.cvLpd[(long long)a.G * s + g] = ok ? -0.91893853320467274178 * m + 0.5 * a.logdet[b] - 0.5 * a.quad[b] : NAN;
}

void launch_kfold_gram(const KfoldArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0 || a.mt <= 0) return;
    static DeviceOnce once;
    lds_opt_in(once, (const void*)kfold_gram_kernel, KF_LDS_BYTES);
    hipLaunchKernelGGL(kfold_gram_kernel, dim3(a.mt * (a.mt + 1) / 2, nbatch), dim3(KF_THREADS), KF_LDS_BYTES, st, a);
}
void launch_kfold_finish(const KfoldArgs& a, int nbatch, hipStream_t st) {
    if (nbatch <= 0 || a.mt <= 0) return;
    hipLaunchKernelGGL(kfold_finish_kernel, dim3(a.mt, nbatch), dim3(GP_TS), 0, st, a);
}
