// What the MFMA tile kernels share (k_tilegemm.hip, k_grad.hip): the K loop's slab geometry, barrier and staging offsets, and the
// persistent work loop — a launch's work items are split over the eight XCDs and dealt inside each XCD by a ticket counter.
#pragma once
#include "gpslc_internal.h"

// The trailing-update kernel raises its waves' issue priority around the 64 MFMAs of a slab (s_setprio 1) and drops it for
// the staging stores, the barrier and the next loads: the wave that HAS MFMAs ready wins the issue slot over its partner's
// staging instructions.  Measured (profiles/r04_ab_experiments.md §11, three alternating pairs): trailing update 66.4 ->
// 67.2 TFLOP/s, unit A +0.55 %; priority 3 the same; on the strip kernel -0.3 % (its second phase wants the partner's
// staging to proceed) -> applied to tile_gemm_nt_kernel only.
// K-loop barriers of every kernel here (trailing, strip, diagonal-tile update) order LDS traffic only: __syncthreads() carries a fence that also waits
// vmcnt(0), i.e. for the slab requested at the top of the iteration — the register staging then ran ONE slab ahead, not two.
// The barrier needs exactly two things, both LDS: this wave's ds_writes of the next slab have landed (lgkmcnt(0)) and every
// wave has issued the MFMAs that consumed its ds_reads of the buffer about to be overwritten (program order before s_barrier).
// Measured (profiles/r04_ab_experiments.md §13): trailing update 66.9 -> 67.2 TFLOP/s, unit A +0.3 %, N = 1024 0..+1.7 %.
#define KLOOP_BARRIER asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define MFMA_PRIO_UP __builtin_amdgcn_s_setprio(1)
#define MFMA_PRIO_DOWN __builtin_amdgcn_s_setprio(0)

#define KS 16
#define LROW 144                      // padded k-row (doubles)
#define OPER_LDS (KS * LROW)          // doubles per operand per stage
#define GEMM_LDS_BYTES (2 * 2 * OPER_LDS * 8)

template <int NEG>
__device__ __forceinline__ d4 mfma_step(double a, double b, d4 c) {
    // blgp bit 0 = negate the MFMA A operand (f64 MFMA re-uses BLGP as NEG[2:0])
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, NEG);
}

// staging: a slab of one operand is 16 KiB = 1024 16-byte chunks, contiguous in HBM, 4 per thread (chunk q = tid + 256 u);
// loff[u] = where chunk q goes in the padded LDS slab (k-row q >> 6, row pair q & 63)
__device__ __forceinline__ void stage_offsets(int tid, int (&loff)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u;
        loff[u] = (q >> 6) * LROW + (q & 63) * 2;
    }
}

// Persistent, XCD-aware work split: XCD x (blockIdx % 8) owns the x-th contiguous run of the launch's W work items.
struct XcdSplit {
    int xcd, local;      // this workgroup's XCD and its rank among the XCD's workgroups
    int gx;              // workgroups on this XCD
    long long x0, xc;    // first item of this XCD's run, items in the run
};
__device__ __forceinline__ XcdSplit xcd_split(long long W) {
    const int G = gridDim.x;
    XcdSplit x;
    x.xcd = blockIdx.x & 7;
    x.local = blockIdx.x >> 3;
    x.gx = (G >> 3) + (x.xcd < (G & 7) ? 1 : 0);
    const long long wq = W >> 3, wrm = W & 7;
    x.x0 = x.xcd * wq + (x.xcd < wrm ? x.xcd : wrm);
    x.xc = wq + (x.xcd < wrm ? 1 : 0);
    return x;
}

// Work distribution inside the XCD's run: the first item of a workgroup is `local`; the following ones come from a per-XCD
// ticket counter (g.queue: GemmArgs::queue, GradArgs::queue) — items differ in cost (augmented-row tiles, skipped diagonal tiles), a static stride
// leaves the slowest workgroup ~5 items behind the mean.  The ticket for the NEXT item is requested at the start of the
// current one, so its latency hides behind the tile.  item_body(item) runs one work item (a tile of a batch element); the
// barrier that ends an item's last slab protects the LDS buffers, the two here the ticket word.
template <class Args, class Body>
__device__ __forceinline__ void ticket_loop(const Args& g, long long W, int tid, Body&& item_body) {
    const XcdSplit x = xcd_split(W);
    __shared__ int s_ticket;
    long long it = x.local;
    while (it < x.xc) {
        int ticket = 0;
        if (tid == 0) ticket = atomicAdd(&g.queue[x.xcd], 1);
        item_body(x.x0 + it);
        if (tid == 0) s_ticket = ticket;
        __syncthreads();
        it = (long long)x.gx + s_ticket;
        __syncthreads();
    }
    // the last workgroup of the XCD to leave re-arms the counters for the next launch on this stream
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(&g.queue[8 + x.xcd], 1) == x.gx - 1) {
            g.queue[x.xcd] = 0;
            g.queue[8 + x.xcd] = 0;
        }
    }
}
