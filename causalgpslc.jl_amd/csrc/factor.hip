// factor.h's definitions: the profiled launch of the tile kernels and the factorisation schedules built from it.
#include "factor.h"

#include <algorithm>
#include <atomic>

namespace gpslc_host {

// the tile kernels leave their ticket counters zeroed; a factorisation re-arms them anyway so that an aborted launch (device
// error in an earlier call) can never make a later one skip work items
void rearm_queue(StreamSlot& s) { HC(hipMemsetAsync(s.queue, 0, 16 * sizeof(int), s.st)); }

// ---- profiled launch of the tile kernels ------------------------------------------------
// a launch description (tile_launch.h) on its stream slot: the slot's ticket counters, no measurement variant
GemmArgs on_slot(GemmArgs g, const StreamSlot& s) { g.diag_skip = 0; g.dbg = nullptr; g.queue = s.queue; return g; }

// prof_base: the kernel class of the profiled launches (0 = class 0 or 1 by the launch's shape)
void gemm(gpslc_ctx* c, const GemmArgs& g0, StreamSlot& s, int prof_base) {
    hipStream_t st = s.st;
    GemmArgs g = on_slot(g0, s);
    if (g.ntiles <= 0 || g.nbatch <= 0 || (g.k1 <= g.k0 && !g.fuse)) return;     // fuse with an empty K range: panel product only
#ifdef GPSLC_DIAG
    // measurement build only: timing-only kernel variants (results are garbage by construction) and in-kernel
    // stamps of one trailing update, written to gpurun_out/gemm_dbg.bin
    static const int diag_skip = diag_env("GPSLC_GEMM_DIAG", 0);
    g.diag_skip = diag_skip;
    static const int dbg_m = diag_env("GPSLC_GEMM_DBG", 0);
    static bool dbg_done = false;
    StampCapture stamps;
    // GPSLC_GEMM_DBG_FUSEK=<K>: the first FUSED in-panel launch whose K loop is K tiles deep instead
    static const int dbg_fk = diag_env("GPSLC_GEMM_DBG_FUSEK", -1);
    const bool dbg_fused = dbg_fk >= 0 && g.fuse && (g.k1 - g.k0) == dbg_fk;
    if (!dbg_done && ((dbg_fk < 0 && dbg_m > 0 && g.shape == 0 && g.mi == dbg_m) || dbg_fused)) {
        g.dbg = stamps.arm((size_t)g.ntiles * g.nbatch * 8);
        dbg_done = true;
    }
#endif
    {
        const bool prof = (c->flags & GPSLC_FLAG_PROFILE) != 0;       // ProfScope does nothing without it
        ProfScope ps(c, prof_base ? prof_base : (g.fuse ? 1 : 0), prof ? tile_launch_flop(g, g.diag_skip) : 0.0, st);
        launch_tile_gemm(g, st);
    }
    // symmetric launches: the full-size diagonal tiles (those above the augmented rows) go to the lower-triangle kernel; those of
    // a fused launch factor_panels updated before it (launch_diag_update_potrf)
    if (!g.fuse && g.sym && g.i0 == g.j0 && (g.diag_skip == 0 || g.diag_skip == 3)) {
        GemmArgs d = g;
        const int cand = g.shape == 0 ? g.mi : 1;      // a column update holds one diagonal tile
        d.mi = g.short_rows > 0 ? std::max(0, std::min(cand, g.short_row0 - g.i0)) : cand;
        launch_syrk_diag(d, g.sym == 3 && g.short_rows > 0 && g.diag_skip == 0, st);
    }
    HC(hipGetLastError());   // launch-configuration errors (LDS opt-in, grid) surface here, not at the end of the call
#ifdef GPSLC_DIAG
    if (stamps.words) {
        FILE* f = fopen("gpurun_out/gemm_dbg.bin", "wb");
        stamps.dump(st, f);
    }
#endif
}

// the device copy of tri_order_pairs(m) (tile_launch.h), made once per ctx and m; null for m <= 2 (tri_decode's order serves)
const unsigned short* tri_order(gpslc_ctx* c, int m) {
    if (m <= 2) return nullptr;
    if ((int)c->tri_order.size() <= m) c->tri_order.resize(m + 1);
    if (c->tri_order[m]) return c->tri_order[m];
    const std::vector<unsigned short> h = tri_order_pairs(m);
    DevBuffer<unsigned short> d;        // kept only once the upload has succeeded
    d.reserve(h.size() * sizeof(unsigned short));
    HC(hipMemcpy(d, h.data(), h.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    return c->tri_order[m] = std::move(d);
}

// ---- the persistent factorisation launch (potrf_tasks_kernel, k_tilegemm.hip): task order = build_task_list, task_list.h ----
namespace {
const TaskList& task_list_for(gpslc_ctx* c, int nt, int back, int nb, int G, int rows, bool aug_full) {
    for (auto& t : c->task_lists)
        if (t.nt == nt && t.back == back && t.nb == nb && t.G == G && t.rows == rows && t.aug_full == aug_full) { t.used = ++c->task_clock; return t; }
    if (c->task_lists.size() >= 8) {       // evict the least recently used shape (nothing of it may still be in flight)
        size_t v = 0;
        for (size_t i = 1; i < c->task_lists.size(); ++i)
            if (c->task_lists[i].used < c->task_lists[v].used) v = i;
        DeviceMem::quiesce();
        c->task_lists.erase(c->task_lists.begin() + (long)v);
    }
    TaskList t;
    t.nt = nt; t.back = back; t.nb = nb; t.G = G; t.rows = rows; t.aug_full = aug_full;
    std::vector<unsigned> h = build_task_list(nt, back, nb, G, rows, aug_full, &t.ntasks);
    t.dev.reserve(h.size() * sizeof(unsigned));
    HC(hipMemcpy(t.dev, h.data(), h.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    t.used = ++c->task_clock;
    c->task_lists.push_back(std::move(t));
    return c->task_lists.back();
}
}  // namespace

// the persistent launch serves: one left-looking panel over the whole width (nt <= task_max_nt), the inverse-based
// factorisation, ONE short augmented row whose tiles ride with the diagonal tasks and whose diagonal tile nobody reads
// (EpiArgs::from_rows) — the shape of run_predict's factorisation of A at N <= 128 task_max_nt
bool potrf_tasks_ok(const gpslc_ctx* c, int nt, int ntot, int short_rows, bool skip_aug_diag, int nb, const double* inv) {
    // one left-looking panel only: a panel width given through gpslc_set_tuning keeps its meaning (nt beyond it takes the panel
    // schedule); with the default width the persistent launch factorises the whole matrix as ONE panel up to task_max_nt
    const int pmax = c->panel_set ? std::max(1, c->panel) : TASK_MAX_NT;
    if (!inv || nt < std::max(2, c->task_min_nt) || nt > std::min(std::min(c->task_max_nt, TASK_MAX_NT), pmax) ||
        nb >= TASK_MAX_BATCH || nb < c->task_min_batch)
        return false;
    return ntot == nt + 1 && short_rows > 0 && short_rows <= GP_TS && skip_aug_diag;
}

// back_alpha (optional, [nb][nt 128]): every matrix's task chain ends with its back-substitution alpha = L^-T z (z = right-hand
// side 0 after the forward solve the factorisation carries): launch_backsolve's result, bit for bit.  The caller checks the
// time-out word when its streams have drained (check_task_timeout).
void potrf_tasks(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, double* inv, int* info, int info_base, int nb, int short_rows,
                 double* back_alpha) {
    hipStream_t st = s.st;
    rearm_queue(s);
    const size_t ints = TASK_SYNC_HDR + (size_t)TASK_SYNC_STRIDE * nb;
    s.sync.reserve(ints * sizeof(int));
    const int mt = task_aug_blocks(short_rows);     // 0: the augmented row is a tile row of the list, not a rider of the diagonal tasks
    const TaskList& tl = task_list_for(c, nt, back_alpha ? 1 : 0, nb, c->task_group,
                                       std::max(1, std::min(4, nt > 8 ? 1 : c->task_rows)), /*aug_full=*/mt == 0);
    HC(hipMemsetAsync(s.sync, 0, ints * sizeof(int), st));
    PotrfTaskArgs a{};
    a.g = task_matrix(M, inv_ref(inv, nt), nt, short_rows, nb, info, info_base);
    a.list = tl.dev; a.sync = s.sync; a.timeout = c->task_timeout; a.nt = nt; a.alpha = back_alpha;
    a.fence_mode = diag_env("GPSLC_TASK_FENCE", 0x30);      // measurement build: bit 0 = no release fence (WRONG results: the
                                                            // price of the fence), bits 4..5 = priority of the diagonal tasks
    c->task_used = true;
    const double Np = (double)nt * GP_TS;
#ifdef GPSLC_DIAG
    // measurement build, GPSLC_TASK_FENCE bit 7: bit 6 (the withheld publish of the time-out test) applies to the first persistent
    // launch of the process only — the later chunks of the same call run normally (tests/test_gpu_tasks.py)
    if (a.fence_mode & 0x80) {
        static std::atomic<int> launches{0};
        if (launches.fetch_add(1) > 0) a.fence_mode &= ~0x40;
        a.fence_mode &= ~0x80;
    }
    // measurement build, GPSLC_TASK_DBG=<n>: per-task stamps of the n-th launch -> gpurun_out/task_dbg.bin (tools/task_stamps.py)
    static const int dbg_at = diag_env("GPSLC_TASK_DBG", 0);
    static int dbg_seen = 0;
    StampCapture stamps;
    if (dbg_at > 0 && ++dbg_seen == dbg_at) a.dbg = stamps.arm((size_t)tl.ntasks * 8);
#endif
    {
        ProfScope ps(c, 4, (Np * Np * Np / 3.0 + (double)a.g.short_rows * Np * Np) * (double)nb, st);
        launch_potrf_tasks(a, tl.ntasks, mt, st);
    }
    HC(hipGetLastError());
#ifdef GPSLC_DIAG
    if (stamps.words) {
        FILE* f = fopen("gpurun_out/task_dbg.bin", "wb");
        stamps.dump(st, f);
    }
#endif
}

// after the call's streams have drained: the ctx's time-out word, read and cleared (no launch zeroes it).  A time-out inside any
// persistent factorisation launch since the last read (any chunk, any stream slot) is an internal error
void check_task_timeout(gpslc_ctx* c) {
    if (!c->task_used) return;
    c->task_used = false;
    int w = 0;
    HC(hipMemcpy(&w, c->task_timeout, sizeof(int), hipMemcpyDeviceToHost));
    if (w == 0) return;
    HC(hipMemset(c->task_timeout, 0, sizeof(int)));
    throw std::runtime_error("persistent factorisation launch timed out waiting for a producer task");
}

// at the start of a call: a previous call that threw between its persistent launches and check_task_timeout (a HIP error, an
// allocation failure) left the time-out word unread — drain what it left in flight and clear the word, so that it neither fails
// this call nor lets its launches stop waiting for their producers
void reset_stale_task_timeouts(gpslc_ctx* c) {
    if (!c->task_used) return;
    for (auto& s : c->slots) HC(hipStreamSynchronize(s.st));
    c->task_used = false;
    HC(hipMemset(c->task_timeout, 0, sizeof(int)));
}

// Blocked Cholesky of the lower-packed nt x nt tile matrix M for near-singular matrices (CovITE + 1e-10 I, SigmaU with its 1e-13
// jitter): no multiplication by an inverted block anywhere — the diagonal tile and the panel below it are solved by substitution
// (k_robust.hip); the column and trailing updates stay on the MFMA tile kernel (a product is backward stable whatever the
// conditioning).  Panels as in factor_panels.  prof_base: see gemm.
void factor_robust(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, int* info, int info_base, int nb, int prof_base) {
    const int pw = std::max(1, c->panel);
    rearm_queue(s);
    for (int k = 0; k < nt; ++k) {
        const int ka = (k / pw) * pw;
        const int kend = std::min(ka + pw, nt);
        if (k > ka) gemm(c, tile_column(M, M, M, k, k, nt - k, ka, k, nb, true), s, prof_base);
        launch_diag_robust(M, k, info, info_base, nb, s.st);
        launch_trsm_robust(M, M, k, k + 1, nt - k - 1, nb, s.st);
        if (k == kend - 1 && nt - kend > 0)
            gemm(c, tile_triangle(M, M, M, kend, nt - kend, ka, kend, nb, tri_order(c, nt - kend)), s, prof_base);
    }
    HC(hipGetLastError());
}

// Blocked Cholesky of the leading nt x nt tiles of the lower-packed ntot x ntot tile matrix M (inverted diagonal blocks into inv);
// the rows nt..ntot-1 are carried along (augmented rows): after the call they hold R = rows * L^-T and the trailing (ntot-nt)^2
// block its Schur complement.  Panels of `pw` tile columns: left-looking inside a panel, one right-looking trailing update
// (K = pw*128) per panel.  prof_base: see gemm.
void factor_panels(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, int ntot, double* inv, int* info, int info_base, int nb,
                   int aug_rows, bool skip_aug_diag, int prof_base) {
    hipStream_t st = s.st;
    // aug_rows > 0: the tile rows nt.. hold only that many live rows in total (right-hand sides);
    // a single augmented tile row is the common case and the only one the kernel shortens
    const int short_rows = (aug_rows > 0 && ntot == nt + 1) ? aug_rows : 0;
    const int pw = std::max(1, c->panel);
    rearm_queue(s);
    const TRef invref = inv_ref(inv, nt);
    for (int k = 0; k < nt; ++k) {
        const int ka = (k / pw) * pw;
        const int kend = std::min(ka + pw, nt);
        const int below = ntot - k - 1;      // tiles of column k below the diagonal
        // the column's strip launch, rows [i0, ntot): update over the panel columns [ka, k), fused with the panel product or not
        auto column = [&](int i0, int k0, bool sym) {
            return short_aug_row(tile_column(M, M, M, i0, k, ntot - i0, k0, k, nb, sym), nt, short_rows);
        };
        if (k > ka && below > 0) {
            // in-panel update: the diagonal tile first — update, factor and inverse in ONE launch — then ONE pass over the column:
            // tile(i,k) -= sum_{kk in [ka,k)} tile(i,kk) tile(k,kk)^T and tile(i,k) *= inv(L_kk)^T for every tile below the
            // diagonal (the column makes one HBM round trip instead of two)
            const GemmArgs g = fused(column(k, ka, true), invref, k);
            GemmArgs d = g;       // the diagonal-tile launch reads the strip's column, K range, F and augmented row (not its fuse)
            d.info = info; d.info_base = info_base;
            launch_diag_update_potrf(d, g.sym == 3, st);
            gemm(c, g, s, prof_base);
        } else {
            // the last column of a matrix without augmented rows (ntot == nt: likelihood_distribution_impl) inside a panel:
            // nothing lies below the diagonal, the column update holds the diagonal tile alone
            if (k > ka) gemm(c, column(k, ka, true), s, prof_base);
            launch_diag(M, k, inv, invref.bstride, info, info_base, nb, st);
            // the first column of a panel has no column update: its panel product tile(i,k) *= inv(L_kk)^T runs as the strip
            // kernel's second phase alone (empty K range: the tile goes from HBM into the accumulators, the fragments of
            // inv(L_kk) from L2 into registers, no LDS staging)
            if (below > 0) gemm(c, fused(column(k + 1, k, false), invref, k), s, prof_base);
        }
        // skip_aug_diag (single short augmented row, epilogue sums from the rows of R): the augmented diagonal tile is
        // never updated — after the last panel it would be the launch's only item
        const bool skip_gd = skip_aug_diag && short_rows > 0;
        if (k == kend - 1 && ntot - kend > (skip_gd ? 1 : 0))     // trailing update with the whole panel
            gemm(c, short_aug_row(tile_triangle(M, M, M, kend, ntot - kend, ka, kend, nb, tri_order(c, ntot - kend)), nt, short_rows,
                                  skip_gd), s, prof_base);
    }
}

}  // namespace gpslc_host
