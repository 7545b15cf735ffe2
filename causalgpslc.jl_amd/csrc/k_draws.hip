// Predictive draws (unit C): the operand staging, the streaming draw kernel and the level-sweep scatter.
// gfx950 only.
#include "gpslc_internal.h"
#include "philox.h"

// ---------------------------------------------------------------------------------------
// Predictive draws: ite[l, i, s*spp + d] = MeanITE_i + (L_c z)_i  (src/estimation.jl:95-109 with the
// factor computed once per (sample, level) instead of once per draw), the library's own normals from philox.h.
// The draws of one unit as a triangular matrix product on the f64 MFMA:  out[:, d] = mu + L_c z[:, d] for up to 128 draws d of
// the unit in one pass over L_c, as a PURE STREAM of L_c (the reference's default is 10 draws; NQ = 1, 2, 4 or 8 blocks of 16
// draws per pass; a unit of more than 128 draws takes one pass per 128, launch_draws).  A lane owns two rows of a tile (r0 =
// 32 wave + 2 (lane & 15) and r0 + 1): it fetches them of a column with ONE 16-byte load straight from HBM (every element of
// L_c is used by exactly one wave, so it never goes through LDS) and stores its two results with one 16-byte store.  MFMA
// operands: A = z (draw index = lane & 15), B = L_c (row = lane & 15), k = lane >> 4, so D[draw = 4v + (lane >> 4)][row = lane & 15].
// HBM-bound up to 32 draws per pass, MFMA-bound beyond.
//   * the pass's normals are laid out ONCE, by draws_zstage_kernel, as the MFMA A-operand image zt: the 16-byte word of
//     lane (lq, li) for the column groups (2m, 2m + 1) of a 32-column chunk sits at lane-contiguous addresses, so a wave
//     fetches its z operands with four fully coalesced 1 KiB loads per chunk — no LDS, no barrier, no dependence
//     between the waves of a workgroup (draws beyond the pass's count and columns >= n are zeros in the image);
//   * a workgroup owns the tile-row PAIR (nt-1-p, p): every item streams nt + 1 tiles, whatever p;
//   * wave w reads only the columns of the diagonal tile at or left of its own 32 rows (8 (w + 1) of the 32 groups);
//   * three register sets of 4 factor loads + 2 z loads each (16-column chunks) in rotation, the next two chunks in flight
//     under the current chunk's MFMAs, 104 VGPRs -> four workgroups per CU; factor loads carry the non-temporal hint (each
//     line is used exactly once).  Measured (same box, 64 units x 10 draws at N = 4096): 6.04 TB/s of factor stream;
//     32-column chunks with two sets 5.6, and the number of workgroups per CU (2 / 3 / 4) does not matter.
// The kernel this replaced (rounds 2-5: z staged in LDS per 64 columns between two barriers, its own normals_kernel; 4.30 TB/s
// at 10 draws, 0.46 at 128, profiles/r05_ab_experiments.md §5; last in commit 4a62acd) issued the same MFMAs with the same
// operands in the same ascending order of k groups, one accumulator per draw: the draws are bit-identical whatever NQ and
// whatever pass a draw falls into (skipped groups of the diagonal tile only ever added +-0;
// tests/test_gpu_draws_parent_bits.py).
// ---------------------------------------------------------------------------------------
// index of z[column g][draw d] in a unit's operand image (16 * Np doubles)
__host__ __device__ inline long long draws_zt_index(long long g, int d) {
    return ((g >> 3) << 7) + ((g & 3) << 5) + ((long long)d << 1) + ((g >> 2) & 1);
}

// one thread = one 16-byte word of the image of a pass (draws a.d0 .. a.d0 + a.nd - 1 of the unit): columns g0 = 8 blk + lq and
// g0 + 4, draw d = a.d0 + dd.  z and the Philox element e = g + n d are indexed by the draw of the UNIT
__global__ __launch_bounds__(256) void draws_zstage_kernel(DrawArgs a) {
    const long long b = blockIdx.y, sb = b / a.lc, lb = b % a.lc;
    const long long s = a.s0 + sb, lev = a.l + lb;
    const long long n = a.n, Np = (long long)a.nt * GP_TS;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;      // word t of the image; block q of 16 draws = words [q 8 Np, ...)
    const int nq = draws_nq(a.nd);               // the stream kernel's NQ: every one of its blocks is written (zeros beyond nd)
    if (t >= Np * 8 * nq) return;
    const long long tq = t % (Np * 8);
    const int dd = (int)(tq & 15) + 16 * (int)(t / (Np * 8)), lq = (int)(tq >> 4) & 3;
    const int d = a.d0 + dd;
    const long long g0 = ((tq >> 6) << 3) + lq, g1 = g0 + 4;
    double v0 = 0.0, v1 = 0.0;
    if (dd < a.nd) {
        if (a.z) {
            const double* __restrict__ zu = a.z + n * a.spp * (s + a.S * lev);
            if (g0 < n) v0 = zu[g0 + n * d];
            if (g1 < n) v1 = zu[g1 + n * d];
        } else if ((n & 1) == 0) {
            // n even: the elements e = g + n d and e ^ 1 of a unit's stream share one Philox counter and one Box-Muller
            // transform (even -> cos, odd -> sin), and the lane that holds column g ^ 1 of the same draw is lane ^ 16 (lq ^ 1).
            // The even-lq lane evaluates the pair of g0, the odd-lq lane the pair of g1 = g0 + 4, and they swap the halves:
            // one counter, one log, one sqrt, one sincos per lane instead of two of each — the same values philox_normal()
            // returns element by element.  (Whole waves reach this point together: Np * 8 * nq is a multiple of 64.)
            const unsigned long long stream = (unsigned long long)((a.rs0 + sb) + a.rS * lev);
            const bool odd = (lq & 1) != 0;
            const long long ge = odd ? (g1 & ~1ll) : g0;            // the even column of the pair this lane evaluates
            double c = 0.0, sn = 0.0;
            if (ge < n) {
                double rad, ang;
                philox_box_muller(a.seed, stream, (unsigned long long)(ge + n * d) >> 1, rad, ang);
                c = rad * cos(ang);
                sn = rad * sin(ang);
            }
            // even-lq lane: keeps cos as its v0 (column g0), sends sin to the partner's v0 (column g0 + 1);
            // odd-lq lane: keeps sin as its v1 (column g1), sends cos to the partner's v1 (column g1 - 1)
            const double give = odd ? c : sn;
            const double got = __shfl_xor(give, 16, 64);
            if (odd) { v0 = got; v1 = sn; } else { v0 = c; v1 = got; }
            if (g0 >= n) v0 = 0.0;
            if (g1 >= n) v1 = 0.0;
        } else {
            const unsigned long long stream = (unsigned long long)((a.rs0 + sb) + a.rS * lev);
            if (g0 < n) v0 = philox_normal(a.seed, stream, (unsigned long long)(g0 + n * d));
            if (g1 < n) v1 = philox_normal(a.seed, stream, (unsigned long long)(g1 + n * d));
        }
    }
    *reinterpret_cast<d2*>(a.zt + b * Np * 16 * nq + 2 * t) = (d2){v0, v1};
}

// CC columns per chunk (CC / 4 k groups of the 16x16x4 MFMA), NS register sets in rotation, WPE waves per SIMD the
// register allocation is held to
template <int CC, int NS, int WPE, int NQ = 1>
__global__ __launch_bounds__(256, WPE) void draws_stream_kernel(DrawArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4;
    const long long b = blockIdx.y, sb = b / a.lc, lb = b % a.lc;      // batch element = (sample, level) pair
    const long long s = a.s0 + sb, lev = a.l + lb;
    const long long n = a.n;
    const long long Np = (long long)a.nt * GP_TS;
    const double* __restrict__ zt = a.zt + b * Np * 16 * NQ + 2 * lane;      // block q of 16 draws: + q * 16 Np
    const int r0 = 32 * wave + 2 * li;                  // this lane's two rows inside the tile: r0, r0 + 1
    const int p = blockIdx.x;
    constexpr int NL = CC / 4, NZ = CC / 8;             // 16-byte factor / z loads per chunk and lane

    for (int half = 0; half < 2; ++half) {
        const int ib = half == 0 ? a.nt - 1 - p : p;
        if (half == 1 && 2 * p == a.nt - 1) break;      // odd nt: the middle row has no partner
        // the tiles (ib, 0..ib) of a row are contiguous in both tile layouts
        const double* __restrict__ Lrow = tref_tile(a.Lc, b, ib, 0) + r0 + lq * GP_TS;
        const int nch = (GP_TS / CC) * ib + (32 / CC) * wave + 32 / CC;   // chunks up to and including the wave's diagonal block
        d4 acc0[NQ], acc1[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { acc0[q] = (d4){0.0, 0.0, 0.0, 0.0}; acc1[q] = acc0[q]; }
        d2 lv[NS][NL], zv[NS][NQ * NZ];
        auto load = [&](int c, d2 (&l)[NL], d2 (&z)[NQ * NZ]) {
            c = min(c, nch - 1);                         // past the end: the last chunk again (keeps the loop body branch-free)
            const double* __restrict__ zp = zt + (long long)c * (CC * 16);
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int m = 0; m < NZ; ++m) z[q * NZ + m] = *reinterpret_cast<const d2*>(zp + q * (16 * Np) + m * 128);
            const double* __restrict__ lp = Lrow + (long long)c * (CC * GP_TS);
#pragma unroll
            for (int kk = 0; kk < NL; ++kk)
                l[kk] = __builtin_nontemporal_load(reinterpret_cast<const d2*>(lp + kk * 4 * GP_TS));
        };
        auto compute = [&](const d2 (&l)[NL], const d2 (&z)[NQ * NZ]) {
#pragma unroll
            for (int kk = 0; kk < NL; ++kk)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double zf = (kk & 1) ? z[q * NZ + (kk >> 1)].y : z[q * NZ + (kk >> 1)].x;
                    acc0[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(zf, l[kk].x, acc0[q], 0, 0, 0);
                    acc1[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(zf, l[kk].y, acc1[q], 0, 0, 0);
                }
        };
        // the chunks of the wave's own 32 x 32 diagonal block: only the lower triangle belongs to L_c
        auto mask_diag = [&](d2 (&l)[NL], int c) {
            const int cb = (c * CC) & 31;                // first column of the chunk relative to the wave's first row
#pragma unroll
            for (int kk = 0; kk < NL; ++kk) {
                const int cc = cb + 4 * kk + lq;
                if (cc > 2 * li) l[kk].x = 0.0;
                if (cc > 2 * li + 1) l[kk].y = 0.0;
            }
        };
        constexpr int ND = 32 / CC;                      // chunks of the diagonal block (1 or 2)
#pragma unroll
        for (int i = 0; i < NS; ++i) load(i, lv[i], zv[i]);
        int c = 0;
        for (; c + NS + ND - 1 < nch; c += NS) {         // chunks c .. c + NS - 1 are all left of the diagonal block
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                compute(lv[i], zv[i]);
                load(c + NS + i, lv[i], zv[i]);
            }
        }
        const int rem = nch - c;                         // ND .. NS + ND - 1 chunks left; the first min(rem, NS) are loaded
#pragma unroll
        for (int i = 0; i < NS + ND - 1; ++i) {
            if (i < rem) {
                if (i >= NS) load(c + i, lv[i % NS], zv[i % NS]);
                if (i >= rem - ND) mask_diag(lv[i % NS], c + i);
                compute(lv[i % NS], zv[i % NS]);
            }
        }
        // acc{0,1}[q][v]: row r0 + {0,1}, draw 16 q + 4 v + lq
        const long long gi = (long long)ib * GP_TS + r0;
        if (gi < n) {
            const double mu0 = a.mean[gi + n * (s + a.S * lev)];
            const double mu1 = (gi + 1 < n) ? a.mean[gi + 1 + n * (s + a.S * lev)] : 0.0;
            double* __restrict__ ob = a.out + a.obase + sb * a.osb + lb * a.osl + gi * a.osi + a.d0 * a.osd;   // the pass's first draw
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int dd = 16 * q + 4 * v + lq;
                if (dd < a.nd) {
                    double* o = ob + (long long)dd * a.osd;
                    const double x0 = mu0 + acc0[q][v], x1 = mu1 + acc1[q][v];
                    if (a.osi == 1 && gi + 1 < n && ((reinterpret_cast<unsigned long long>(o) & 15ull) == 0)) {
                        *reinterpret_cast<d2*>(o) = (d2){x0, x1};
                    } else {
                        o[0] = x0;
                        if (gi + 1 < n) o[a.osi] = x1;
                    }
                }
            }
        }
    }
}

// Level sweep (L > 1): the draws of the sub-batch are produced level by level into tmp[b][l][d][i] (instance
// fastest: coalesced stores) and rearranged ONCE into the reference's level-fastest tensor
// ite[l + L*(i + n*(s*spp + d))] (src/prediction.jl:30-33) through LDS, so that both the reads (1 KiB runs along i)
// and the writes (runs along l) are contiguous.
#define SC_LC 32
__global__ __launch_bounds__(256) void draws_scatter_kernel(const double* __restrict__ tmp, double* __restrict__ out,
                                                            long long n, int L, int spp, long long s0) {
    __shared__ double tl[SC_LC][GP_TS + 1];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * GP_TS;
    const int d = blockIdx.y;
    const long long b = blockIdx.z;
    const double* src = tmp + ((b * L) * spp + d) * n;                                // + l*spp*n + i
    double* dst = out + (long long)L * n * ((s0 + b) * spp + d);                       // + l + L*i
    for (int l0 = 0; l0 < L; l0 += SC_LC) {
        const int nl = min(SC_LC, L - l0);
        __syncthreads();
        for (int idx = tid; idx < SC_LC * GP_TS; idx += 256) {
            const int ll = idx >> 7, ii = idx & 127;
            if (ll < nl && i0 + ii < n) tl[ll][ii] = src[(long long)(l0 + ll) * spp * n + i0 + ii];
        }
        __syncthreads();
        for (int idx = tid; idx < SC_LC * GP_TS; idx += 256) {
            const int ll = idx & (SC_LC - 1), ii = idx / SC_LC;
            if (ll < nl && i0 + ii < n) dst[(l0 + ll) + (long long)L * (i0 + ii)] = tl[ll][ii];
        }
    }
}

template <int CC, int NS, int WPE, int NQ>
static void launch_stream(const DrawArgs& a, int nbatch, hipStream_t st) {
    hipLaunchKernelGGL((draws_stream_kernel<CC, NS, WPE, NQ>), dim3((a.nt + 1) / 2, nbatch), dim3(256), 0, st, a);
}
// passes of up to 128 draws, each one pass over L_c: the pass's operand image, then the stream kernel of its block count
void launch_draws(const DrawArgs& unit, int nbatch, hipStream_t st) {
    DrawArgs a = unit;
    for (a.d0 = 0; a.d0 < a.spp; a.d0 += 128) {
        a.nd = min(128, a.spp - a.d0);
        const int nq = draws_nq(a.nd);
        const long long words = (long long)a.nt * GP_TS * 8 * nq;
        hipLaunchKernelGGL(draws_zstage_kernel, dim3((unsigned)((words + 255) / 256), nbatch), dim3(256), 0, st, a);
        // more than 16 draws: NQ z blocks and accumulator pairs per wave.  HBM-bound up to 32 draws, MFMA-bound beyond (the
        // factor is still read exactly once): fewer, fatter waves.
        // register-set arrangements tried at NQ = 1 (profiles/r05_ab_experiments.md §1): <32,2,2> 5.62-5.65 TB/s, <32,2,3> 5.59,
        // <32,3,2> 5.55, <16,4,3> 5.60, <16,4,4> 6.02, <16,3,4> 6.04 (this one) on one box; 5.5-5.6 for every one of them on another
        switch (nq) {
            case 1: launch_stream<16, 3, 4, 1>(a, nbatch, st); break;
            case 2: launch_stream<16, 3, 3, 2>(a, nbatch, st); break;
            case 4: launch_stream<16, 3, 2, 4>(a, nbatch, st); break;
            default: launch_stream<16, 2, 1, 8>(a, nbatch, st); break;
        }
    }
}
void launch_draws_scatter(const double* tmp, double* out, long long n, int L, int spp, long long s0, int nbatch,
                          hipStream_t st) {
    hipLaunchKernelGGL(draws_scatter_kernel, dim3((unsigned)((n + GP_TS - 1) / GP_TS), spp, nbatch), dim3(256), 0, st,
                       tmp, out, n, L, spp, s0);
}
