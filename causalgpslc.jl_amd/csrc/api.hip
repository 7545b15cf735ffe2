// Host side of libgpslc_hip.so: context, workspace, chunk scheduling over HIP streams, and the
// C ABI of include/gpslc_hip.h.  No exception crosses the ABI (everything is caught and mapped to
// a status code); every HIP error is reported through gpslc_last_error.
#include "../../include/gpslc_hip.h"
#include "gpslc_internal.h"
#include "batch_plan.h"
#include "tile_launch.h"
#include "dev_mem.h"
#include "sm_layout.h"
#include "philox.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace {

struct HipFail {
    hipError_t e;
    const char* what;
    int line;
};
#define HC(x)                                                         \
    do {                                                              \
        hipError_t _e = (x);                                          \
        if (_e != hipSuccess) throw HipFail{_e, #x, __LINE__};        \
    } while (0)

// The two memory policies of dev_mem.h.  A failed allocation also clears the runtime's sticky error.
struct DeviceMem {
    static void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    static void release(void* p) { (void)hipFree(p); }
    static void quiesce() { HC(hipDeviceSynchronize()); }
};
struct PinnedMem {      // pinned, device-visible host memory
    static void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    static void release(void* p) { (void)hipHostFree(p); }
    static void quiesce() { HC(hipDeviceSynchronize()); }
};
template <class T = char> using DevBuffer = Buffer<DeviceMem, T>;
using PinnedBuffer = Buffer<PinnedMem>;

// a HIP stream, owned: stands where its hipStream_t stood
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// the two HIP events around one profiled launch region, owned
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() = default;
    EventPair(EventPair&& o) noexcept : a(std::exchange(o.a, nullptr)), b(std::exchange(o.b, nullptr)) {}
    EventPair& operator=(EventPair&& o) noexcept { std::swap(a, o.a); std::swap(b, o.b); return *this; }
    ~EventPair() {
        for (hipEvent_t e : {a, b})
            if (e) (void)hipEventDestroy(e);
    }
    bool create() { return hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
};

struct ProfRec {
    EventPair ev;
    double flop;
    int cls;     // kernel class, see gpslc_profile_get_class (include/gpslc_hip.h)
};
constexpr int kProfClasses = 5;

// device-resident task list of one (tile count, augmented row, batch size, group size) shape of the persistent
// factorisation launch (potrf_tasks_kernel); built once per shape and kept (see task_list_for)
struct TaskList {
    int nt = 0, back = 0, nb = 0, G = 0, rows = 0;
    bool aug_full = false;
    DevBuffer<unsigned> dev;
    long long ntasks = 0;
    unsigned long long used = 0;
};

// one HIP stream of a ctx and what its launches use: the chunks of a call alternate over the slots
struct StreamSlot {
    Stream st;
    Arena<DeviceMem> arena;
    DevBuffer<int> queue;          // ticket-counter block (16 ints), see GemmArgs::queue
    DevBuffer<int> sync;           // progress words of the persistent factorisation launch (PotrfTaskArgs::sync), grown on demand
};

// The last dense covariance handed to gpslc_mvn_logpdf / gpslc_mvn_draw (SigmaU is constant per data set).  n <= 640 (both
// paths can run): the matrix itself, always, whichever path the hand-over took; the tiled factor is built from it when a
// call on the tiled path finds it missing or older (tiles_gen != gen).  n > 640: only the tiled factor.
struct MvnCache {
    DevBuffer<double> tiles;     // tiled factor (substitution-based: no inverted diagonal blocks are kept)
    DevBuffer<double> dense;     // n <= 640: the dense covariance itself (the single-workgroup path refactorises it in LDS)
    uint64_t gen = 0;            // hand-overs so far
    uint64_t tiles_gen = 0;      // the hand-over `tiles` was factorised from (0 = none)
    double logdet = 0.0;         // of `tiles`
    int info = 0;                // LAPACK-style info of the latest covariance
    bool valid = false;
};

}  // namespace

struct gpslc_ctx {
    int device = 0;
    int64_t n = 0;
    int nX = 0, nU = 0;
    uint32_t flags = 0;
    int nt = 0;
    DevBuffer<double> dX, dT, dY;
    bool has_data = false;
    bool binary_t = false;   // every treatment is exactly 0 or 1 (detected in gpslc_set_data)
    int max_batch = 0;   // 0 = auto
    int panel = 8;
    bool panel_set = false;        // gpslc_set_tuning gave a panel width: the persistent launch then serves nt <= panel only
    int64_t ens_off = 0, ens_S = 0;   // gpslc_set_ensemble: placement of a call's samples for the Philox stream ids
    int nstreams = 1;   // chunks of one call alternate over this many HIP streams (2 buys ~1-2 %, see profiles/)
    std::vector<StreamSlot> slots;   // one per stream (ensure_streams)
    // persistent factorisation launch (potrf_tasks_kernel): cached task lists, the time-out word every launch of the ctx sets
    // when a poll exceeds its bound, and whether a call has used it (the word is then checked when the call's streams have drained)
    std::vector<TaskList> task_lists;
    unsigned long long task_clock = 0;
    DevBuffer<int> task_timeout;
    bool task_used = false;        // a persistent launch ran since the time-out word was last read (check_task_timeout)
    int task_min_nt = 2, task_max_nt = TASK_MAX_NT;   // tile counts in this range take the persistent launch (128 < N <= 4096: with
                                            // groups of 32 it wins at every tile count the descriptor can hold — N = 256 +1..3 %, 384 +6 %, 512 +10 %,
                                            // 1024 +6 %, 1536 +4 %, 2048 +2.4 %, 3072 +1.8 %, 4096 +1.0..1.3 % against panels of 8 + trailing
                                            // updates, profiles/r06_ab_experiments.md §1d)
    int task_min_batch = 256;      // ... when the chunk holds at least this many matrices: a persistent launch over few
                                   // matrices is a chain of hand-offs (N = 1024: 2.1 ms for 8 matrices against 1.5 ms with one
                                   // launch per column; even at 256, profiles/r06_ab_experiments.md §1)
    int task_group = 32;           // matrices per group of the task order (see build_task_list)
    int task_rows = 2;             // consecutive tile rows of a column per strip task up to 8 tiles per side (beyond: one — long K
                                   // loops amortise the task's fetch / acquire / publish by themselves, and finer tasks balance
                                   // better: N = 1536 .. 4096 +0.6 .. 1.2 %, profiles/r06_ab_experiments.md §1d)
    Arena<DeviceMem> scratch;      // call-level buffers (internal MeanITE of a draws-only call, ...)
    PoolArena<DeviceMem> io;       // staging of the host-pointer entry points and per-call info words
    // single-launch small-n node scores (k_small.hip): pinned, device-visible host staging (descriptors, inputs,
    // results) and host copies of the ctx's data for assembling the :Y node's feature block
    PinnedBuffer pin;
    // two pinned bounce chunks for large device -> pageable-host hand-overs (copy_out_large), allocated on first use
    PinnedBuffer bounce[2];
    std::vector<double> hX, hT, hY;
    std::vector<double> stage_f, stage_rest;   // host staging of gpslc_nodes_logpdf's batched pass (grown, never shrunk)
    std::string err;
    std::vector<int32_t> last_info;
    MvnCache mvn;
    // L2-blocked visiting orders of the lower-triangular tile sets, keyed by the triangle size m
    std::vector<DevBuffer<unsigned short>> tri_order;
    // profiling of the dominant kernel
    std::vector<ProfRec> prof;
    size_t prof_used = 0;
    int64_t prof_launches[kProfClasses] = {};     // per kernel class, see ProfRec::cls
    double prof_ms[kProfClasses] = {}, prof_flop[kProfClasses] = {};
};

namespace {

void set_err(gpslc_ctx* c, const std::string& s) {
    if (c) c->err = s;
}

// HIP events around a launch region on `st` (GPSLC_FLAG_PROFILE only): accumulates into kernel class `cls`
struct ProfScope {
    gpslc_ctx* c;
    ProfRec* r = nullptr;
    hipStream_t st;
    ProfScope(gpslc_ctx* c_, int cls, double work, hipStream_t st_) : c(c_), st(st_) {
        if (!(c->flags & GPSLC_FLAG_PROFILE)) return;
        if (c->prof_used == c->prof.size()) {
            ProfRec n{};
            if (!n.ev.create()) return;
            c->prof.push_back(std::move(n));
        }
        r = &c->prof[c->prof_used++];
        r->flop = work;
        r->cls = cls;
        (void)hipEventRecord(r->ev.a, st);
    }
    ~ProfScope() { if (r) (void)hipEventRecord(r->ev.b, st); }
};

int fail_hip(gpslc_ctx* c, const HipFail& f) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) at api.hip:%d in `%s`", (int)f.e, hipGetErrorString(f.e),
             f.line, f.what);
    set_err(c, buf);
    return GPSLC_ERR_HIP;
}

void ensure_streams(gpslc_ctx* c) {
    if (!c->task_timeout) {
        DevBuffer<int> w;
        w.reserve(sizeof(int));
        HC(hipMemset(w, 0, sizeof(int)));
        c->task_timeout = std::move(w);
    }
    while ((int)c->slots.size() < c->nstreams) {
        StreamSlot s;       // joins the ctx complete or not at all
        HC(hipStreamCreateWithFlags(&s.st.s, hipStreamNonBlocking));
        s.queue.reserve(16 * sizeof(int));
        HC(hipMemset(s.queue, 0, 16 * sizeof(int)));
        c->slots.push_back(std::move(s));
    }
}

// the tile kernels leave their ticket counters zeroed; a factorisation re-arms them anyway so that an aborted launch (device
// error in an earlier call) can never make a later one skip work items
void rearm_queue(StreamSlot& s) { HC(hipMemsetAsync(s.queue, 0, 16 * sizeof(int), s.st)); }

// ---- profiled launch of the tile kernels ------------------------------------------------
#ifdef GPSLC_DIAG
// measurement build only: the in-kernel stamps of one launch.  arm() hands the kernel a zeroed buffer of 8-byte words; after the
// launch, where armed (words != 0), dump() waits for it and writes the words to the file its caller opened (null: nothing is
// written); the buffer goes with the capture
struct StampCapture {
    DevBuffer<unsigned long long> buf;
    size_t words = 0;
    unsigned long long* arm(size_t n) {
        buf.reserve(std::max<size_t>((words = n) * 8, 8));
        HC(hipMemset(buf, 0, n * 8));
        return buf;
    }
    void dump(hipStream_t st, FILE* file) {
        std::unique_ptr<FILE, int (*)(FILE*)> f(file, fclose);      // closed on every way out
        HC(hipStreamSynchronize(st));
        std::vector<unsigned long long> h(words);
        HC(hipMemcpy(h.data(), buf, words * 8, hipMemcpyDeviceToHost));
        if (f) fwrite(h.data(), 8, words, f.get());
    }
};
#endif

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

void prof_collect(gpslc_ctx* c) {
    for (size_t i = 0; i < c->prof_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->prof[i].ev.a, c->prof[i].ev.b) == hipSuccess) {
            const int k = c->prof[i].cls;
            c->prof_ms[k] += ms;
            c->prof_flop[k] += c->prof[i].flop;
            c->prof_launches[k] += 1;
        }
    }
    c->prof_used = 0;
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

// One prediction call is described once, by three pieces: the extern "C" entry points fill them with the caller's pointers
// (PredictRequest: host or device, as given) and run_predict reads them with device pointers (PredictIO).
struct Posterior {                   // the S posterior samples of the call
    int64_t S = 0;
    SampleParams p{};                // the six per-sample arrays
};
// What each level form (level_form.h) can be combined with: run_predict's backstop behind the entry points' validate.  A baseline
// is required by the paired form and refused by the others.  Every form takes weights: their rules stay in run_predict.
struct FormRules { int form; const char* name; bool factual, baseline, vec, fp32; };
template <int FORM, typename LF = LevelForm<FORM>>
constexpr FormRules form_row(const char* name) { return {FORM, name, LF::factual, LF::paired, LF::vector_levels, LF::fp32_kernels}; }
constexpr FormRules kFormRules[] = {form_row<FORM_ORDINARY>("ordinary levels"), form_row<FORM_CONTRAST>("contrasts"),
                                    form_row<FORM_SLOPE>("slopes"), form_row<FORM_OUTCOME>("outcomes")};
static const FormRules& form_rules(int form) {
    for (const FormRules& r : kFormRules)
        if (r.form == form) return r;
    throw std::runtime_error("unknown level form");
}

struct Levels {
    int L = 0;
    const double* doT = nullptr;
    bool vec = false;                // vector levels: doT is n x L (level l at doT + n*l), not L scalars
    int form = FORM_ORDINARY;        // FORM_* (level_form.h), set by the entry points
    const double* base = nullptr;    // FORM_CONTRAST (L): level l is doT[l] against base[l]
    void against(const double* b) { base = b; form = b ? FORM_CONTRAST : FORM_ORDINARY; }   // a contrast exactly when a baseline is given
    bool needs_kw() const { return form_rules(form).factual; }     // only the factual term brings K W in
    LevelSet set(int nlevels) const { return LevelSet{doT, base, nlevels, form, vec ? 1 : 0}; }      // what the kernels take
    // weighted effects: G weight columns — the caller's W[i + n*g] on the host, column fastest (W[g + G*j]) on the
    // device; meanSATE / varSATE are then S x L x G — element (s, l, g) at s + S*(l + L*g) — of tau_w = w_g' ITE_l, the weights
    // used as given (scalar levels only)
    int G = 0;
    const double* W = nullptr;
};
struct DrawsAndOutputs {
    double pred_noise = 0;
    int spp = 0;
    uint64_t seed = 0;
    const double* z = nullptr;
    double *meanSATE = nullptr, *varSATE = nullptr, *meanITE = nullptr, *ite_draws = nullptr;
    // weighted calls only: the joint covariance of the L levels per weight column, S x L x L x G — element
    // (s, l, l', g) at s + S*(l + L*(l' + L*g)); needs varSATE, whose values are its diagonal
    double* covW = nullptr;
};

// What the outcome-model calls add to a prediction call: device pointers, null where the output is not asked
struct Loo {                         // leave-one-out predictive checks (gpslc_y_loo): n x S each
    double *mean = nullptr, *var = nullptr, *lpd = nullptr;
    bool any() const { return mean || var || lpd; }
};
struct Lgo {                         // leave-group-out predictive checks (gpslc_y_lgo): n x S, n x S, G x S
    int G = 0, mmax = 0;             // groups; members of the largest
    const int *members = nullptr, *offsets = nullptr;      // the members sorted by (group, row), the G + 1 offsets into them
    double *mean = nullptr, *var = nullptr, *lpd = nullptr;
    bool any() const { return mean || var || lpd; }
};
struct Grad {                        // gradient of the outcome log-likelihood (gpslc_y_logpdf_grad), in the layouts of
    // the arguments they differentiate: U n x nU x S, uyLS nU x S, xyLS nX x S, the others S; Y n x S
    double *U = nullptr, *uyLS = nullptr, *xyLS = nullptr, *tyLS = nullptr, *yScale = nullptr, *yNoise = nullptr, *Y = nullptr;
    bool pairs() const { return U || uyLS || xyLS || tyLS; }     // those that need the pass over the pairs
    bool needs_c() const { return yScale || yNoise; }            // those that need c = diag(A^-1)
    bool any() const { return pairs() || needs_c() || Y; }
};
struct NewIndividuals {              // predictions for m new individuals (gpslc_predict_new)
    const double *Xnew = nullptr, *Unew = nullptr;      // their features: m x nX, m x nU x S
    int m = 0;
    double *mean = nullptr, *var = nullptr, *cov = nullptr;     // m x S x L each and m x m x S x L; cov needs var: its diagonal
    bool pairs() const { return var || cov; }            // the (sample, level) pairs need tile workspace
    bool any() const { return mean || pairs(); }
    // weighted averages over them (gpslc_predict_new_weighted), a call of its own: Levels::W / G are then G weight
    // columns over the m NEW individuals (device: W[g + G*i]) and DrawsAndOutputs::meanSATE / varSATE / covW receive meanW, varW, covW
    bool weighted = false;
};

struct PredictIO {
    Posterior post;
    Levels lv;
    DrawsAndOutputs out;
    const double* X = nullptr;   // device X to use (ctx or override)
    double *logdet = nullptr, *quad = nullptr;
    // ITEDistributions-style outputs (single level): MeanITEs S x n, CovITEs S x n x n
    double *MeanITEs = nullptr, *CovITEs = nullptr;
    int* info = nullptr;   // device, S
    int nU = -1, nX = -1;            // feature counts of this call (default: the ctx's)
    const double* Y = nullptr;       // right-hand side 0 (default: the ctx's Y) and its per-sample stride
    long long y_sstride = 0;
    bool p_shared_u = false;         // the feature block is shared by all samples (u_sstride stays 0)
    int64_t ens_off = 0, ens_S = 0;  // ens_S > 0: this call's placement in a larger ensemble (else the ctx's, gpslc_set_ensemble)
    // node draws (gpslc_nodes_draw beyond the single-workgroup kernels): ndraw[:, s] = chol(A_s) nz[:, s] from the batched
    // tiled factor of A_s (n x S each, device; nzero = n x S zeros, the draw kernel's mean)
    const double* nz = nullptr;
    const double* nzero = nullptr;
    double* ndraw = nullptr;
    Loo loo;
    Lgo lgo;
    Grad grad;
    bool grad_no_t = false;          // node mode of the gradient (GradArgs::no_t): no treatment column
    NewIndividuals fresh;
};

// chunk and unit-B sub-batch sizes of a call (batch_plan.h holds the arithmetic; here: what the schedule would like and what
// the device has)
BatchPlan auto_batch(gpslc_ctx* c, int64_t S, int L, size_t per_sample_bytes, size_t unit_bytes, size_t lvl_extra) {
    // enough matrices in flight that the per-step diagonal-block kernel (one workgroup per matrix) and the
    // launch quantisation of the late, small trailing updates are amortised: 1024 at N = 4096 (82 GB of the
    // 288 GB; measured 2013 / 2040 / 2055 / 2064 samples/s at batch 256 / 512 / 1024 / 2048)
    // small matrices: up to 16,384 per chunk (N = 1024: 4,096 / 8,192 / 16,384 per chunk -> 83.8 k / 84.6 k / 86.5 k samples/s,
    // profiles/r04_ab_experiments.md §16 — every launch's ramp and tail are amortised over more items); memory permitting
    long long b = 1048576LL / ((long long)c->nt * c->nt);
    b = std::max<long long>(32, std::min<long long>(b, 16384));
    if (c->max_batch > 0) b = c->max_batch;
    // unit-B sub-batch (unit_bytes > 0): 128 units at N = 4096 (203 MB each, 26 GB).  Round 5, 256 units of 8 samples x 32 levels
    // on one box (profiles/r05_ab_experiments.md §3): 16 / 32 / 64 / 128 / 256 per sub-batch -> 322 / 349 / 364 / 372 / 373
    // units/s — the late columns of a factorisation have (nt - k) x sub-batch items for 512 workgroup slots; flat from 128 on
    const long long want_bb = std::max<long long>(1, std::min<long long>(128, 131072LL / ((long long)c->nt * c->nt)));
    size_t free_b = 0, tot_b = 0;
    HC(hipMemGetInfo(&free_b, &tot_b));
    size_t have = 0;
    for (auto& sl : c->slots) have += sl.arena.bytes();
    // the AUTOMATIC chunk also stays under 30 % of the device's memory (arenas never shrink, and the host process usually
    // shares the device: torch's caching allocator under sharded.py / bench.py, other contexts of gpslc_predict_multi on one
    // GPU); 1,024 matrices at N = 4096 are 28 %.  gpslc_set_tuning(max_batch) may ask for more: then only what is free counts.
    const BatchPlan p = plan_batch(b, want_bb, S, L, per_sample_bytes, unit_bytes, lvl_extra, free_b, have, tot_b, c->nstreams,
                                   c->max_batch <= 0);
    if (!p.ok) throw std::bad_alloc();
    return p;
}

// what one run_predict call computes and the sizes that follow from it (the same for all of its chunks)
struct PredictShape {
    int n, nt, L, R, naug, ntot;      // R: right-hand sides beside Y — one per level, or L*G with weight columns
    long long Np, tiles_per, nlow;   // padded N, tiles of A with its augmented rows, tiles of an nt x nt triangle
    bool with_sums, want_cov, want_draws, want_mean, unitB;     // unitB: full ITE covariance (CovITE, draws)
    bool want_loo, want_lgo;          // leave-one-out outputs, leave-group-out outputs
    bool want_grad, grad_pairs, grad_c;   // gradient outputs; those that need the pass over the pairs (U and the lengthscales'); those
                                      // that need c = diag(A^-1) (yScale, yNoise)
    bool want_w;                      // W = L^-T is wanted (by any of them)
    bool want_alpha;                  // alpha = A^-1 Y is wanted (by the MeanITE pass or by them)
    int mt;                           // new individuals: their row tiles, the tiles of an mt x mt triangle, and whether the
    long long mlow;                   // (sample, level) pairs need tile workspace (variance, covariance)
    bool want_new, new_pairs;
    PredictShape(const gpslc_ctx* c, const PredictIO& io)
        : n((int)c->n), nt(c->nt), L(io.lv.L), R(io.lv.W ? io.lv.L * io.lv.G : io.lv.L), naug((R + 1 + GP_TS - 1) / GP_TS), ntot(nt + naug),
          Np((long long)nt * GP_TS), tiles_per((long long)ntot * (ntot + 1) / 2), nlow((long long)nt * (nt + 1) / 2),
          with_sums(io.out.meanSATE || io.out.varSATE || io.out.covW), want_cov(io.CovITEs != nullptr), want_draws(io.out.ite_draws != nullptr),
          want_mean(io.out.meanITE || io.MeanITEs || want_draws), unitB(want_cov || want_draws),
          want_loo(io.loo.any()), want_lgo(io.lgo.any()), want_grad(io.grad.any()), grad_pairs(io.grad.pairs()),
          grad_c(io.grad.needs_c()), want_w(want_loo || want_lgo || want_grad), want_alpha(want_mean || want_w || io.fresh.mean),
          mt((io.fresh.m + GP_TS - 1) / GP_TS), mlow((long long)mt * (mt + 1) / 2), want_new(io.fresh.any()),
          new_pairs(io.fresh.pairs()) {}
};

// one chunk of a call: samples s0 .. s0 + nb - 1 on one stream slot, and the buffers carve_chunk takes for it from the slot's arena
struct Chunk {
    StreamSlot* s = nullptr;
    int64_t s0 = 0;
    int nb = 0;
    TRef M{};                        // the tile matrices of A over `tiles`
    double *tiles = nullptr, *inv = nullptr, *part = nullptr, *bsum = nullptr, *ksum = nullptr, *sumdelta = nullptr;
    double *vpart = nullptr, *zwork = nullptr, *znode = nullptr;
    double *bw = nullptr, *kw = nullptr, *wnorm2 = nullptr;      // weighted effects: B W, K W [nb][G][Np], w_g . w_g [nb][G]
    double* cprior = nullptr;        // joint covariance across the levels: beta, kappa, gamma_l [nb][G][L + 2]
    double* wpart = nullptr;         // weighted averages over new individuals: the row blocks' shares of w' B** w [nb][mt][G]
    double *loo_w = nullptr, *loo_c = nullptr;      // leave-one-out: W = L^-T as a packed triangle of tiles [nb][nlow], diag(A^-1) [nb][Np]
    double *grad_ls = nullptr, *grad_u = nullptr;   // gradient: the pair pass's partial sums per tile (GradArgs::part_ls, part_u)
    // unit B: a sub-batch of gs_max samples x lc_max levels; W, CovITE, the draws' normals, level-sweep staging, failure codes
    int lc_max = 0, gs_max = 0;
    double *Wt = nullptr, *Ct = nullptr, *zt = nullptr, *dtmp = nullptr;
    int* pinfo = nullptr;
    SampleGrid grid{};               // the chunk's samples and feature blocks, as every RBF-evaluating kernel takes them
};

struct ChunkBytes { size_t per_sample = 1024, per_pair = 0, per_level = 0; };    // 1 KiB: the 256-byte alignment of each buffer

// Carves a chunk's buffers from its slot's arena (nb samples, sub-batches of Bb pairs) and counts, beside each buffer, the bytes
// auto_batch reserves for it: per sample, per (sample, level) pair of a unit-B sub-batch, and per level of a sweep beyond the
// sub-batch (the level-sweep staging).  ch == nullptr: the counts only.
ChunkBytes carve_chunk(const PredictShape& sh, const PredictIO& io, int Bb, Chunk* ch) {
    ChunkBytes by;
    Chunk none;
    Chunk& b = ch ? *ch : none;
    Arena<DeviceMem>* ar = ch ? &ch->s->arena : nullptr;
    auto take = [&](size_t per_sample) -> double* {
        by.per_sample += per_sample * 8;
        return ar ? ar->take<double>((size_t)b.nb * per_sample) : nullptr;
    };
    const int n = sh.n, nt = sh.nt, L = sh.L;
    // the streaming draw kernel reads a pass's normals (caller's or Philox) from the unit's operand image (DrawArgs::zt)
    const size_t zimage_doubles = sh.want_draws ? draws_image_doubles(io.out.spp, sh.Np) : 0;
    b.tiles = take(sh.tiles_per * GP_TSQ);
    b.inv = take((size_t)nt * GP_TSQ);
    if (sh.with_sums && !io.lv.W) b.part = take(2 * nt * sh.Np);
    b.bsum = take(sh.Np); b.ksum = take(sh.Np);
    b.sumdelta = take(std::max(sh.R, 1));
    if (io.lv.W) {      // only the factual form needs K W
        b.bw = take((size_t)io.lv.G * sh.Np);
        b.kw = io.lv.needs_kw() ? take((size_t)io.lv.G * sh.Np) : b.bw;
        b.wnorm2 = take(io.lv.G);
        if (io.out.covW) b.cprior = take((size_t)io.lv.G * (L + 2));
        if (io.fresh.weighted) b.wpart = take((size_t)sh.mt * io.lv.G);
    }
    if (io.lv.vec && sh.with_sums) b.vpart = take((size_t)L * nt);     // vector levels: per-tile shares of sum(Delta)
    b.zwork = take(2 * sh.Np);                                          // zwork + alpha
    if (io.ndraw) b.znode = take(draws_image_doubles(1, sh.Np));        // operand image of the node draw's normals
    if (sh.want_w) b.loo_w = take((size_t)sh.nlow * GP_TSQ);
    if (sh.want_loo || sh.grad_c) b.loo_c = take(sh.Np);
    if (sh.grad_pairs) {      // F numbers per lower tile; 128 nU per (tile row, tile column)
        b.grad_ls = take((size_t)sh.nlow * (io.nU + io.nX + (io.grad_no_t ? 0 : 1)));
        if (io.nU > 0) b.grad_u = take((size_t)nt * nt * io.nU * GP_TS);
    }
    b.M = lower_ref(b.tiles, sh.tiles_per * GP_TSQ);
    if (sh.new_pairs) {       // new individuals: W* (mt x nt) and, with the covariance, an mt triangle per (sample, level) pair
        const size_t w_tiles = (size_t)sh.mt * nt, c_tiles = io.fresh.cov ? (size_t)sh.mlow : 0;
        by.per_pair = (w_tiles + c_tiles) * GP_TSQ * 8 + 512;
        if (!ar) return by;
        b.lc_max = std::min(L, Bb);
        b.gs_max = std::max(1, Bb / b.lc_max);
        b.Wt = ar->take<double>((size_t)Bb * w_tiles * GP_TSQ);
        if (c_tiles) b.Ct = ar->take<double>((size_t)Bb * c_tiles * GP_TSQ);
        return by;
    }
    if (!sh.unitB) return by;
    by.per_pair = (size_t)((long long)nt * nt + sh.nlow) * GP_TSQ * 8;
    if (sh.want_draws) {
        by.per_pair += zimage_doubles * 8 + 256 + (L > 1 ? (size_t)io.out.spp * n * 8 + 256 : 0) + sizeof(int) + 256;
        by.per_level = (size_t)io.out.spp * n * 8;
    }
    if (!ar) return by;
    b.lc_max = std::min(L, Bb);                      // levels per sub-batch
    b.gs_max = std::max(1, Bb / b.lc_max);           // samples per sub-batch
    b.Wt = ar->take<double>((size_t)Bb * nt * nt * GP_TSQ);
    b.Ct = ar->take<double>((size_t)Bb * sh.nlow * GP_TSQ);
    // draws: the operand images of one sub-batch, and for a level sweep the staging buffer
    // [sample][level][d][i] that is rearranged into the level-fastest tensor sample group by group (per unit of the sub-batch:
    // max(1, Bb / L) samples x L levels <= Bb pairs, or one sample's L > Bb levels — per_level)
    if (sh.want_draws) b.zt = ar->take<double>((size_t)Bb * zimage_doubles);
    if (sh.want_draws && L > 1) b.dtmp = ar->take<double>((size_t)b.gs_max * L * io.out.spp * n);
    // failure codes of the CovITE factors, one per pair of a sub-batch (folded into io.info after each sub-batch)
    if (sh.want_draws) b.pinfo = ar->take<int>((size_t)Bb);
    return by;
}

// the vector-level kernels' arguments of a chunk (doT is n x L: level l at doT + n*l)
VecArgs vec_args(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    VecArgs va{ch.grid};
    va.lv = io.lv.set(sh.L);
    va.M = ch.M; va.part = ch.vpart; va.sumdelta = ch.sumdelta;
    va.Y = io.Y; va.y_sstride = io.y_sstride;
    return va;
}

// One draw per unit from N(0, L L^T): unit b streams the factor Lc of batch element b (batch stride 0: ONE factor for all) and
// multiplies it with column s0 + b of the normals z (n x S); `zero` is n x S zeros (the draw kernel's mean), zt the operand
// image workspace, out n x S.
DrawArgs zero_mean_draw(TRef Lc, int n, int nt, long long s0, long long S, const double* zero, const double* z, double* zt,
                        double* out) {
    DrawArgs dr{};
    dr.Lc = Lc; dr.n = n; dr.nt = nt; dr.s0 = s0; dr.S = S; dr.l = 0; dr.lc = 1; dr.L = 1; dr.spp = 1;
    dr.mean = zero; dr.z = z; dr.zt = zt; dr.out = out;
    dr.obase = (long long)n * s0; dr.osb = n; dr.osl = 0; dr.osi = 1; dr.osd = n;
    return dr;
}

// unit A of a chunk: Gram build, right-hand sides, vector sums, factorisation, epilogue and node draw.  Returns whether the
// factorisation delivered the back-substitution alpha.
bool unit_a(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nt = sh.nt, nb = ch.nb;
    const int64_t s0 = ch.s0;
    GramArgs ga{ch.grid};
    ga.M = ch.M; ga.part = ch.part;
    ga.with_sums = (sh.with_sums && !io.lv.W) ? 1 : 0;      // weighted: the column sums come from launch_wsum instead
#ifdef GPSLC_DIAG
    static const int gram_dbg = diag_env("GPSLC_GRAM_DBG", 0);
    static bool gram_dbg_done = false;
    StampCapture stamps;
    if (gram_dbg && !gram_dbg_done) ga.dbg = stamps.arm((size_t)8 * nb * (nt * (nt + 1) / 2));
#endif
    ga.f32 = (c->flags & GPSLC_FLAG_FP32_KERNEL) ? 1 : 0;
    ga.binary_t = (c->binary_t && io.nU == c->nU && io.nX == c->nX && io.Y == c->dY) ? 1 : 0;   // ctx data only
    const bool over_new = io.fresh.weighted;      // the weight columns run over the new individuals
    if (over_new) {     // B*' W over the m x n pairs, w' B** w over the m x m pairs, and the sums the prepare kernels would form
        NewWsumArgs wa{};
        static_cast<SampleGrid&>(wa) = ch.grid;
        wa.Xnew = io.fresh.Xnew; wa.Unew = io.fresh.Unew; wa.un_sstride = (long long)io.fresh.m * io.nU; wa.m = io.fresh.m; wa.mt = sh.mt;
        wa.lv = io.lv.set(sh.L); wa.G = io.lv.G; wa.W = io.lv.W;
        wa.bw = ch.bw; wa.part = ch.wpart; wa.sumdelta = ch.sumdelta; wa.wnorm2 = ch.wnorm2; wa.prior = ch.cprior;
        launch_new_wsum(wa, nb, st);
    } else if (io.lv.W) {      // weighted effects: B W and K W, one pass over the pairs for all columns and levels (independent of the tiles)
        WsumArgs wa{ch.grid};
        wa.G = io.lv.G; wa.W = io.lv.W;
        wa.bw = ch.bw; wa.kw = ch.kw; wa.with_k = io.lv.needs_kw() ? 1 : 0; wa.binary_t = ga.binary_t;
        launch_wsum(wa, nb, st);
    }
    launch_gram(ga, nb, st);
#ifdef GPSLC_DIAG
    if (ga.dbg) {      // GPSLC_GRAM_DBG: dump the first launch's per-workgroup stamps
        FILE* f = fopen("gpurun_out/gram_dbg.bin", "wb");
        stamps.dump(st, f);
        gram_dbg_done = true;
    }
#endif
    RhsArgs ra{};
    ra.T = c->dT; ra.Y = io.Y; ra.y_sstride = io.y_sstride; ra.tyLS = io.post.p.tyLS; ra.s0 = s0;
    // vector levels: rhs_tiles writes zeros into the level rows and rhs_prepare no level sums (no levels here); launch_vec_sums
    // fills both below
    ra.lv = io.lv.set((sh.with_sums && !io.lv.vec) ? sh.L : 0);
    ra.n = n; ra.nt = nt; ra.naug = sh.naug; ra.with_sums = sh.with_sums ? 1 : 0;
    ra.part = ch.part; ra.bsum = ch.bsum; ra.ksum = ch.ksum; ra.sumdelta = ch.sumdelta; ra.M = ch.M;
    const bool epi_rows = (sh.naug == 1);                    // single augmented tile row: the epilogue sums from the rows of R
    const int live = (sh.with_sums ? sh.R : 0) + 1;          // right-hand sides: Y and one c_l per level (and weight column)
    ra.live_rows = (epi_rows && live <= 32) ? 16 * ((live + 15) / 16) : 0;
    ra.G = 1; ra.bw = ch.bsum; ra.kw = ch.ksum;       // the plain call: one column of level sums, the Gram build's
    if (io.lv.W) { ra.W = over_new ? nullptr : io.lv.W; ra.G = io.lv.G; ra.bw = ch.bw; ra.kw = ch.kw; ra.wnorm2 = ch.wnorm2; }
    launch_rhs(ra, nb, st, over_new);
    if (io.lv.vec && sh.with_sums) launch_vec_sums(vec_args(io, sh, ch), nb, st);
    // NB: the MeanITE pass takes K alpha as Y - yNoise alpha (k_solve.hip, ite_mean_kernel): it relies on alpha solving EXACTLY
    // (K_gram + yNoise I) alpha = Y.  Any future jitter, robust fallback or different right-hand side in this factorisation must
    // be reflected there (tests: test_mean_ite_tiny_noise_and_near_coincident_levels).
    const int short_rows = sh.naug == 1 ? live : 0;
    bool back_done = false;
    if (potrf_tasks_ok(c, nt, sh.ntot, short_rows, epi_rows, nb, ch.inv)) {
        // small tile counts: the whole factorisation (and the back-substitution) as ONE persistent launch of tile tasks
        potrf_tasks(c, *ch.s, ch.M, nt, ch.inv, io.info + s0, 0, nb, short_rows,
                    sh.want_alpha ? ch.zwork + (long long)nb * sh.Np : nullptr);
        back_done = sh.want_alpha;
    } else {
        factor_panels(c, *ch.s, ch.M, nt, sh.ntot, ch.inv, io.info + s0, 0, nb, live, epi_rows, 0);
    }
    EpiArgs ea{};
    ea.M = ch.M; ea.n = n; ea.nt = nt; ea.naug = sh.naug; ea.L = sh.with_sums ? sh.R : 0; ea.s0 = s0; ea.S = io.post.S;
    ea.sumdelta = ch.sumdelta; ea.pred_noise = io.out.pred_noise;
    ea.meanSATE = io.out.meanSATE; ea.varSATE = io.out.varSATE; ea.logdet = io.logdet; ea.quad = io.quad;
    ea.from_rows = epi_rows ? 1 : 0;
    if (io.lv.W) { ea.wnorm2 = ch.wnorm2; ea.wL = sh.L; }
    launch_epilogue(ea, nb, st);
    if (io.out.covW) {      // the levels' joint covariance per weight column: Gram matrix of the rows the factorisation carried
        CurveArgs ca{};
        ca.M = ch.M; ca.n = n; ca.nt = nt; ca.lv = io.lv.set(sh.L); ca.G = io.lv.G; ca.s0 = s0; ca.S = io.post.S;
        ca.T = c->dT; ca.tyLS = io.post.p.tyLS;
        ca.W = io.lv.W; ca.bw = ch.bw; ca.kw = ch.kw; ca.prior = ch.cprior;
        ca.varW = io.out.varSATE; ca.covW = io.out.covW;
        launch_curve(ca, nb, st, over_new);
    }
    if (io.ndraw) {
        // one draw from N(0, A_s) per parameter set with the caller's normals: L_s z_s on the factor just computed — Gen's
        // mvnormal(zeros(n), cov) of an elliptical slice's auxiliary vector (src/inference.jl:225-232) and of the :logitT prior
        // draw (src/model_likelihood.jl:25-33) — the predictive-draw kernel streaming L once
        launch_draws(zero_mean_draw(ch.M, n, nt, s0, io.post.S, io.nzero, io.nz, ch.znode, io.ndraw), nb, st);
    }
    return back_done;
}

// alpha = A^-1 Y of a chunk where the factorisation did not deliver it: the back-substitution
void back_substitute(const PredictShape& sh, const Chunk& ch) {
    BackArgs ba{};
    ba.M = ch.M; ba.inv = ch.inv; ba.inv_bstride = (long long)sh.nt * GP_TSQ; ba.nt = sh.nt; ba.naug = sh.naug; ba.zwork = ch.zwork;
    launch_backsolve(ba, ch.nb, ch.s->st);
}

// MeanITE of a chunk from alpha: the ITE-mean kernels, once per output layout asked for: meanITE n x S x L, MeanITEs S x n (the
// reference layout, single level)
void mean_ite(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nb = ch.nb;
    const double* alpha = ch.zwork + (long long)nb * sh.Np;
    const long long S = io.post.S;
    const struct { double* out; long long si, ss, sl; } outs[2] = {{io.out.meanITE, 1, n, (long long)n * S}, {io.MeanITEs, S, 1, 0}};
    if (io.lv.vec) {
        VecArgs va = vec_args(io, sh, ch);
        va.alpha = alpha;
        for (const auto& o : outs)
            if (o.out) { va.meanITE = o.out; va.si = o.si; va.ss = o.ss; va.sl = o.sl; launch_vec_mean(va, nb, st); }
        return;
    }
    IteMeanArgs ia{ch.grid};
    ia.S = S; ia.lv = io.lv.set(sh.L); ia.alpha = alpha;
    ia.Y = io.Y; ia.y_sstride = io.y_sstride; ia.yNoise = io.post.p.yNoise;
    ia.f32 = (c->flags & GPSLC_FLAG_FP32_KERNEL) ? 1 : 0;
    for (const auto& o : outs)
        if (o.out) { ia.meanITE = o.out; ia.si = o.si; ia.ss = o.ss; ia.sl = o.sl; launch_ite_mean(ia, nb, st); }
}

// unit B's W <- D L^-T for ub (sample, level) pairs, left-looking over the whole width: one strip launch per tile column (column
// update + panel product with inv(L_kk)^T in the same work item; column 0 takes the panel product alone), which measured level
// with blocking it like the factorisation (profiles/r04_ab_experiments.md §7).  W has `rows` tile rows: nt for unit B's D, the
// row tiles of the new individuals for D* (unit_new).
void w_solve(gpslc_ctx* c, StreamSlot& s, const TRef& W, const TRef& Ls, const TRef& invref, int nt, int ub, int rows) {
    for (int k = 0; k < nt; ++k) gemm(c, fused(tile_column(W, Ls, W, 0, k, rows, 0, k, ub, false), invref, k), s, 3);
}

// what LooArgs, LgoArgs and GradArgs share: the chunk's W = L^-T, alpha = A^-1 Y, the scored Y and the samples' failure codes
template <class Args>
Args on_w(const PredictIO& io, const PredictShape& sh, const Chunk& ch, Args a = Args{}) {
    a.W = ch.loo_w; a.w_bstride = sh.nlow * GP_TSQ; a.n = sh.n; a.nt = sh.nt; a.s0 = ch.s0;
    a.alpha = ch.zwork + (long long)ch.nb * sh.Np; a.Y = io.Y; a.y_sstride = io.y_sstride; a.info = io.info;
    return a;
}

// Leave-one-out predictive checks of a chunk: c = diag(A^-1) as the squared row norms of W = L^-T, then the
// outputs from alpha, c and Y; and / or its leave-group-out checks (§20) from the same W and alpha.  The gradient (§21, grad() below) reads W,
// alpha and c as this function leaves them.  W is built block diagonal by block diagonal, one launch each: diagonal d holds the tiles
// (i, i + d) of all tile rows and matrices, each a chain of d tile products from kk = i on (nt^3/6 products in all, the
// factorisation's count); the tile rows of a matrix are independent chains, so nt x nb of them are in flight.
void loo(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int nt = sh.nt, nb = ch.nb;
    LooArgs la = on_w<LooArgs>(io, sh, ch);
    la.inv = ch.inv; la.inv_bstride = (long long)nt * GP_TSQ;
    la.S = io.post.S; la.c = ch.loo_c;
    la.looMean = io.loo.mean; la.looVar = io.loo.var; la.looLpd = io.loo.lpd;
    HC(hipMemsetAsync(ch.loo_w, 0, sizeof(double) * (size_t)nb * sh.nlow * GP_TSQ, st));     // every chain starts from a zero tile
    launch_loo_init(la, nb, st);
    rearm_queue(*ch.s);
    const TRef W = lower_ref(ch.loo_w, la.w_bstride), invref = inv_ref(ch.inv, nt);
    // a fused column of nt - d items; the kernel gives item i its own tile (i, i + d), K range and inverted block
    for (int d = 1; d < nt; ++d)
        launch_loo_diagonal(on_slot(fused(tile_column(W, ch.M, W, 0, 0, nt - d, 0, 0, nb, false), invref, 0), *ch.s), nt, d, st);
    if (sh.want_loo || sh.grad_c) launch_loo_rownorm(la, nb, st);
    if (sh.want_loo) launch_loo_finish(la, nb, st);
    if (sh.want_lgo) {      // leave-group-out: one workgroup per (group, sample) on the same W and alpha
        LgoArgs ga = on_w<LgoArgs>(io, sh, ch);
        ga.G = io.lgo.G; ga.mmax = io.lgo.mmax; ga.members = io.lgo.members; ga.offsets = io.lgo.offsets;
        ga.lgoMean = io.lgo.mean; ga.lgoVar = io.lgo.var; ga.lgoLpd = io.lgo.lpd;
        launch_lgo_groups(ga, nb, st);
    }
    HC(hipGetLastError());
}

// Gradient of the outcome log-likelihood of a chunk, after loo() has left W, alpha and, where asked, c: the pass
// over the lower tiles of A^-1 = W W^T (nt^3/6 tile products, the factorisation's count) when U's or a lengthscale's gradient is
// asked, then the kernel that adds the tiles' partial sums and writes every output.  gyScale, gyNoise and gY alone need no pair pass.
void grad(const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    GradArgs ga = on_w(io, sh, ch, GradArgs{ch.grid});
    ga.S = io.post.S; ga.c = ch.loo_c;
    ga.part_ls = ch.grad_ls; ga.part_u = ch.grad_u; ga.queue = ch.s->queue;
    ga.dU = io.grad.U; ga.duyLS = io.grad.uyLS; ga.dxyLS = io.grad.xyLS; ga.dtyLS = io.grad.tyLS;
    ga.dyScale = io.grad.yScale; ga.dyNoise = io.grad.yNoise; ga.dY = io.grad.Y;
    ga.no_t = io.grad_no_t ? 1 : 0;
    if (sh.grad_pairs) {
        rearm_queue(*ch.s);
        launch_grad_pairs(ga, ch.nb, st);
    }
    launch_grad_finish(ga, ch.nb, st);
    HC(hipGetLastError());
}

// The pair workspaces of a chunk (unit B's CovITE, the new individuals' variance and covariance) batch over (posterior sample,
// level) PAIRS: a sub-batch is gs samples x lc levels (gs * lc = ub <= Bb), batch element b = (sample g0 + b / lc, level l0 +
// b % lc).  Every pair has its own tiles; the factor of A (Ls) and its inverted diagonal blocks (invref) are shared by a
// sample's levels (TRef::bdiv = lc) — the shape of predictCounterfactualEffects (src/prediction.jl:30-33): few samples, ~100 levels.
template <class Body>
void for_pair_batches(const PredictShape& sh, const Chunk& ch, Body&& body) {
    const long long bstride = sh.tiles_per * GP_TSQ, inv_bs = (long long)sh.nt * GP_TSQ;
    for (int g0 = 0; g0 < ch.nb; g0 += ch.gs_max) {
        const int gs = std::min(ch.gs_max, ch.nb - g0);
        for (int l0 = 0; l0 < sh.L; l0 += ch.lc_max) {
            const int lc = std::min(ch.lc_max, sh.L - l0);
            TRef Ls = lower_ref(ch.tiles + (long long)g0 * bstride, bstride);
            TRef invref = inv_ref(ch.inv + (long long)g0 * inv_bs, sh.nt);
            Ls.bdiv = invref.bdiv = lc;
            body(g0, gs, l0, lc, gs * lc, Ls, invref);
        }
    }
}

// C <- C - W W^T on the lower tiles of C's `rows` tile rows, for ub pairs (W: rows x nt tiles)
void minus_w_wt(gpslc_ctx* c, StreamSlot& s, const TRef& W, const TRef& C, int nt, int ub, int rows) {
    gemm(c, tile_triangle(W, W, C, 0, rows, 0, nt, ub, tri_order(c, rows)), s, 3);
}

// Unit B of a chunk: the full ITE covariance of every pair, W <- D L^-T, CovITE (+ jitter) = Delta - W W^T, and what is asked of
// it: the covariance itself, or draws from it
void unit_b(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int n = sh.n, nt = sh.nt, L = sh.L;
    const int64_t s0 = ch.s0;
    const TRef W = rect_ref(ch.Wt, (long long)nt * nt * GP_TSQ, nt), Cm = lower_ref(ch.Ct, sh.nlow * GP_TSQ);
    for_pair_batches(sh, ch, [&](int g0, int gs, int l0, int lc, int ub, const TRef& Ls, const TRef& invref) {
        DtArgs da{ch.grid};
        da.s0 = s0 + g0;
        da.lv = io.lv.set(L); da.l0 = l0; da.lc = lc;
        da.pred_noise = io.out.pred_noise; da.W = W; da.Cm = Cm;
        launch_dt_build(da, ub, st);
        w_solve(c, *ch.s, W, Ls, invref, nt, ub, nt);
        minus_w_wt(c, *ch.s, W, Cm, nt, ub, nt);
        if (sh.want_cov) {       // ITEDistributions: single level (lc == 1)
            GatherCovArgs gc{};
            gc.Cm = Cm; gc.n = n; gc.nt = nt; gc.s0 = s0 + g0; gc.S = io.post.S; gc.out = io.CovITEs;
            launch_gather_cov(gc, ub, st);
        }
        if (!sh.want_draws) return;
        // one failure code per pair, then per sample the code of its lowest-index failing level (the reference's loop
        // order, src/prediction.jl:30-33): a shared word per sample would let the lc levels of a diagonal launch race,
        // and the lowest failing tile column win across launches
        HC(hipMemsetAsync(ch.pinfo, 0, sizeof(int) * ub, st));
        factor_robust(c, *ch.s, Cm, nt, ch.pinfo, n, ub, 3);
        launch_fold_pair_info(ch.pinfo, io.info + s0 + g0, gs, lc, st);
        DrawArgs dr{};
        dr.Lc = Cm; dr.n = n; dr.nt = nt; dr.s0 = s0 + g0; dr.S = io.post.S; dr.l = l0; dr.lc = lc; dr.L = L;
        dr.spp = io.out.spp; dr.mean = io.out.meanITE; dr.z = io.out.z; dr.zt = ch.zt; dr.seed = io.out.seed;
        const int64_t eS = io.ens_S > 0 ? io.ens_S : c->ens_S, eo = io.ens_S > 0 ? io.ens_off : c->ens_off;
        dr.rs0 = dr.s0 + (eS > 0 ? eo : 0); dr.rS = eS > 0 ? eS : io.post.S;
        if (L == 1) {     // the reference tensor directly: n x (S*spp), instance fastest
            dr.out = io.out.ite_draws;
            dr.obase = (long long)n * io.out.spp * (s0 + g0); dr.osb = (long long)n * io.out.spp; dr.osl = 0;
            dr.osi = 1; dr.osd = n;
        } else {          // staging [sample][level][d][i]
            dr.out = ch.dtmp;
            dr.obase = (long long)l0 * io.out.spp * n; dr.osb = (long long)L * io.out.spp * n;
            dr.osl = (long long)io.out.spp * n; dr.osi = 1; dr.osd = n;
        }
        {
            ProfScope ps(c, 2, (double)ub * io.out.spp, st);     // unit C: work = draws
            launch_draws(dr, ub, st);
        }
        if (L > 1 && l0 + lc == L)      // the sample group's last levels: its staged draws into the level-fastest tensor
            launch_draws_scatter(ch.dtmp, io.out.ite_draws, n, L, io.out.spp, s0 + g0, gs, st);
    });
}

// Predictions for new individuals of a chunk.  The mean is one pass over the m x n pairs per sample for all
// levels and needs no workspace; variance and covariance batch over (sample, level) pairs like unit B: D*(l) (and prior_l B**)
// into the pair's tiles, W* = D* L^-T against the sample's factor, var from the squared row norms of W*, cov from the lower
// tiles of prior_l B** + pred_noise I - W* W*^T.
void unit_new(gpslc_ctx* c, const PredictIO& io, const PredictShape& sh, const Chunk& ch) {
    hipStream_t st = ch.s->st;
    const int nt = sh.nt, mt = sh.mt, nb = ch.nb;
    const NewIndividuals& f = io.fresh;
    NewArgs na{};
    static_cast<SampleGrid&>(na) = ch.grid;
    na.Xnew = f.Xnew; na.Unew = f.Unew; na.un_sstride = (long long)f.m * io.nU; na.m = f.m; na.mt = mt;
    na.S = io.post.S; na.lv = io.lv.set(sh.L); na.l0 = 0; na.lc = 1; na.pred_noise = io.out.pred_noise;
    na.alpha = ch.zwork + (long long)nb * sh.Np;
    na.mean = f.mean; na.var = f.var; na.cov = f.cov;
    if (f.mean) launch_new_mean(na, nb, st);
    if (sh.new_pairs) {
        na.W = rect_ref(ch.Wt, (long long)mt * nt * GP_TSQ, nt);
        na.Cm = f.cov ? lower_ref(ch.Ct, sh.mlow * GP_TSQ) : TRef{};
        for_pair_batches(sh, ch, [&](int g0, int, int l0, int lc, int ub, const TRef& Ls, const TRef& invref) {
            na.s0 = ch.s0 + g0; na.l0 = l0; na.lc = lc;
            launch_new_build(na, ub, st);
            w_solve(c, *ch.s, na.W, Ls, invref, nt, ub, mt);
            launch_new_var(na, ub, st);
            if (!f.cov) return;
            minus_w_wt(c, *ch.s, na.W, na.Cm, nt, ub, mt);
            launch_new_gather(na, ub, st);
        });
    }
    HC(hipGetLastError());
}

// the chunked ensemble driver (device pointers everywhere)
void run_predict(gpslc_ctx* c, const PredictIO& io_in) {
    PredictIO io = io_in;
    const FormRules& fr = form_rules(io.lv.form);
    const struct { bool refused; const char* why; } refusals[] = {
        {io.lv.vec && !fr.vec, " cannot be combined with vector levels"},
        {(c->flags & GPSLC_FLAG_FP32_KERNEL) && !fr.fp32, " need an fp64 context"},
        {(io.lv.base != nullptr) != fr.baseline, fr.baseline ? " need a baseline" : " cannot be combined with a contrast baseline"}};
    for (const auto& r : refusals)
        if (r.refused) throw std::runtime_error(std::string(fr.name) + r.why);
    if (io.lv.W && io.lv.vec) throw std::runtime_error("weights cannot be combined with vector levels");
    if (io.lv.W && (c->flags & GPSLC_FLAG_FP32_KERNEL)) throw std::runtime_error("weighted effects need an fp64 context");
    if (io.lv.W && io.lv.G < 1) throw std::runtime_error("weights without a weight column");
    if (io.out.covW && (!io.lv.W || !io.out.varSATE)) throw std::runtime_error("the joint covariance needs weights and varW");
    if (io.lv.W && !io.out.meanSATE && !io.out.varSATE) { io.lv.W = nullptr; io.lv.G = 0; }      // nothing weighted is asked for
    if (io.fresh.any()) {
        if (fr.factual) throw std::runtime_error("new individuals have no factual treatment: ordinary levels cannot be predicted for them");
        if (io.lv.vec || io.fresh.m < 1) throw std::runtime_error("new individuals need scalar levels and m >= 1");
        if (io.fresh.cov && !io.fresh.var) throw std::runtime_error("the covariance of new individuals needs their variance: its diagonal");
        if (io.CovITEs || io.out.ite_draws) throw std::runtime_error("new individuals cannot be combined with CovITE or draws: one pair workspace");
    }
    if (io.fresh.weighted) {
        if (fr.factual) throw std::runtime_error("new individuals have no factual treatment: ordinary levels cannot be predicted for them");
        if (!io.lv.W || io.fresh.m < 1) throw std::runtime_error("weighted averages over new individuals need weights and m >= 1");
        if (io.fresh.any() || io.CovITEs || io.out.ite_draws || io.out.meanITE || io.MeanITEs)
            throw std::runtime_error("weighted averages over new individuals are a call of their own: no per-individual outputs, CovITE or draws");
    }
    if (io.nU < 0) io.nU = c->nU;
    if (io.nX < 0) io.nX = c->nX;
    if (!io.Y) { io.Y = c->dY; io.y_sstride = 0; }
    if (io.post.p.u_sstride == 0 && io.nU > 0 && io.post.p.U != nullptr && !io.p_shared_u) io.post.p.u_sstride = (long long)c->n * io.nU;
    reset_stale_task_timeouts(c);
    ensure_streams(c);
    const PredictShape sh(c, io);
    // chunk size and sub-batch from what the device has (the sub-batch's workspace is sized from the pairs the call
    // really has, and the 30 % rule of the automatic chunk covers its per-sample part only)
    const ChunkBytes by = carve_chunk(sh, io, 0, nullptr);
    const BatchPlan plan = auto_batch(c, io.post.S, sh.L, by.per_sample, by.per_pair, by.per_level);
    const int Bt = (int)plan.Bt, Bb = (int)plan.Bb;      // Bb: (sample, level) pairs per unit-B sub-batch, no more than the call has
    const size_t need = (size_t)Bt * by.per_sample + plan.fixed;
    for (int i = 0; i < c->nstreams; ++i) c->slots[i].arena.reserve(need);
    // internal MeanITE buffer when the caller did not ask for it but the draws need it
    if (sh.want_draws && !io.out.meanITE) {
        c->scratch.reserve((size_t)sh.n * io.post.S * sh.L * 8 + (1 << 16));
        c->scratch.reset();
        io.out.meanITE = c->scratch.take<double>((size_t)sh.n * io.post.S * sh.L);
    }
    HC(hipMemsetAsync(io.info, 0, sizeof(int) * io.post.S, c->slots[0].st));
    HC(hipStreamSynchronize(c->slots[0].st));
    int chunk = 0;
    for (int64_t s0 = 0; s0 < io.post.S; s0 += Bt, ++chunk) {
        Chunk ch{&c->slots[chunk % c->nstreams], s0, (int)std::min<int64_t>(Bt, io.post.S - s0)};
        ch.s->arena.reset();
        carve_chunk(sh, io, Bb, &ch);
        ch.grid = SampleGrid{io.X, c->dT, io.post.p, s0, sh.n, io.nX, io.nU, sh.nt};
        const bool back_done = unit_a(c, io, sh, ch);
        if (sh.want_alpha && !back_done) back_substitute(sh, ch);
        if (sh.want_mean) mean_ite(c, io, sh, ch);
        if (sh.want_w) loo(io, sh, ch);
        if (sh.want_grad) grad(io, sh, ch);
        if (sh.unitB) unit_b(c, io, sh, ch);
        if (sh.want_new) unit_new(c, io, sh, ch);
    }
    for (auto& s : c->slots) HC(hipStreamSynchronize(s.st));
    HC(hipGetLastError());
    check_task_timeout(c);
    if (c->flags & GPSLC_FLAG_PROFILE) prof_collect(c);
    c->last_info.resize(io.post.S);
    HC(hipMemcpy(c->last_info.data(), io.info, sizeof(int) * io.post.S, hipMemcpyDeviceToHost));
}

int first_info(const gpslc_ctx* c) {
    for (int32_t v : c->last_info)
        if (v != 0) return v;
    return 0;
}

template <class F>
int guarded(gpslc_ctx* c, F&& f) {
    try {
        if (c) HC(hipSetDevice(c->device));
        return f();
    } catch (const HipFail& h) {
        return fail_hip(c, h);
    } catch (const std::bad_alloc&) {
        set_err(c, "device workspace allocation failed");
        return GPSLC_ERR_NOMEM;
    } catch (const std::runtime_error& e) {
        set_err(c, std::string("internal error: ") + e.what());
        return GPSLC_ERR_INTERNAL;
    } catch (...) {
        set_err(c, "internal error");
        return GPSLC_ERR_INTERNAL;
    }
}

int bad_arg(gpslc_ctx* c, int k, const char* what) {
    char buf[160];
    snprintf(buf, sizeof buf, "argument #%d is invalid: %s", k, what);
    set_err(c, buf);
    return -k;
}

double* up(DevBuffer<double>& b, const double* host, size_t count) {
    b.reserve(std::max<size_t>(count * sizeof(double), 8));
    if (count) HC(hipMemcpy(b, host, count * sizeof(double), hipMemcpyHostToDevice));
    return b;
}
// upload into the ctx's staging pool (no allocation in steady state)
double* up(gpslc_ctx* c, const double* host, size_t count) {
    double* d = c->io.take<double>(count);
    if (count) HC(hipMemcpy(d, host, count * sizeof(double), hipMemcpyHostToDevice));
    return d;
}

// ---- single-launch small-n node scores ----------------------------------------------------------------------------
struct HostNode {            // host view of one node (gpslc_node with plain pointers)
    int nF;
    const double* F[2];      // up to two column groups + one extra column are concatenated into the feature block:
    int nFpart[2];           //   F[0] (nFpart[0] columns), F[1] (nFpart[1] columns), then `col` (one column) if non-null
    const double* col;
    const double* ls[2];     // lengthscales of the two groups; ls_col for the extra column
    double ls_col;
    double scale, noise;
    const double* target;
    const double* dev_cov;   // dense-covariance node: n x n in device memory (else null), and its scale factor
    double covscale;
};

// The three kinds of node view.  An RBF node: K = scale exp(-sum_f ((x_if - x_jf) / ls_f)^2) + noise I over nF feature columns
HostNode rbf_node(int nF, const double* F, const double* ls, double scale, double noise, const double* target) {
    HostNode h{};
    h.nF = nF; h.F[0] = nF ? F : nullptr; h.nFpart[0] = nF; h.ls[0] = nF ? ls : nullptr;
    h.scale = scale; h.noise = noise; h.target = target;
    return h;
}
// the :Y node: the same over the feature parts U | X | T (T one column with the scalar lengthscale tyLS)
HostNode y_node(int nU, const double* U, const double* uyLS, int nX, const double* X, const double* xyLS, const double* T,
                double tyLS, double scale, double noise, const double* target) {
    HostNode h = rbf_node(nU, U, uyLS, scale, noise, target);
    h.nF = nU + nX + 1;
    h.F[1] = nX ? X : nullptr; h.nFpart[1] = nX; h.ls[1] = nX ? xyLS : nullptr;
    h.col = T; h.ls_col = tyLS;
    return h;
}
// a dense-covariance node: K = covscale dev_cov (n x n, device)
HostNode dense_node(const double* dev_cov, double covscale, const double* target) {
    HostNode h{};
    h.dev_cov = dev_cov; h.covscale = covscale; h.target = target;
    return h;
}

// log N(x; 0, K) of an n-vector from log det K and the quadratic form x' K^-1 x
constexpr double kLog2Pi = 1.8378770664093454835606594728112;
inline double gauss_logpdf(size_t n, double logdet, double quad) { return -0.5 * ((double)n * kLog2Pi + logdet + quad); }

// A node score can run as ONE workgroup of one launch: matrix resident in LDS (n <= 160..176), or the left-looking
// kernel with the finished block columns in an L2-resident scratch (n <= 640).  The latter keeps one CU busy per node
// for 100+ us: worth it up to a few hundred nodes per call, beyond that the batched tiled path wins.
bool fast_path_ok(const gpslc_ctx* c, int nF_max, int64_t count) {
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) return false;
    if (small_gp_lds_bytes((int)c->n, nF_max) <= kLdsCapBytes) return count <= 4096;
    return MidLayout::fits((int)c->n) && count <= 512;
}

// Device -> host hand-over of a LARGE result (draw tensors, MeanITE of a level sweep: GB).  A plain hipMemcpy into pageable
// memory runs at ~10 GB/s (the runtime's own bounce copies + first-touch page faults of a fresh destination, on one
// thread) against 57 GB/s of DMA into pinned memory (tools/bench_small_n_predict.py).  Here the DMA of chunk k + 1 into
// one of two pinned chunks overlaps the copy of chunk k into the caller's buffer, and that copy is split over a few
// threads: 1.1 GB in 77 ms instead of 110 (a huge-page hint on the destination changed nothing: NumPy's large arrays
// already carry it).  Small results keep the plain call; a caller who hands over a PINNED buffer gets the DMA rate.
constexpr size_t kBounceBytes = size_t(64) << 20;
// The source is `rows` runs of row_bytes, CONTIGUOUS ON THE DEVICE, that land `dpitch` bytes apart in the caller's array: a
// shard's block of an (n x S x L) array of a level sweep — level l of the shard is one run of n S_r doubles at n (s0 + S l) of
// the caller's array (gpslc_predict_multi).  The device side is DMA'd chunk by chunk whatever the rows; each host thread
// scatters its slice of a chunk to the rows it covers.  rows == 1 or dpitch == row_bytes is one run: one memcpy per slice.
void copy_out_rows(gpslc_ctx* c, void* dst, size_t dpitch, const void* src_dev, size_t row_bytes, size_t rows) {
    if (rows == 0 || row_bytes == 0) return;
    const size_t bytes = row_bytes * rows;
    const bool strided = rows > 1 && dpitch != row_bytes;
    const size_t run = strided ? row_bytes : bytes;
    auto direct = [&]() {
        if (strided) HC(hipMemcpy2D(dst, dpitch, src_dev, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost));
        else HC(hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost));
    };
    bool plain = bytes < 2 * kBounceBytes;
    if (!plain) {                                     // a pinned (registered) destination takes the DMA directly
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst) == hipSuccess) plain = at.type == hipMemoryTypeHost;
        else (void)hipGetLastError();                 // ordinary pageable memory: not known to the runtime
    }
    if (plain) { direct(); return; }
    ensure_streams(c);
    try {
        for (PinnedBuffer& b : c->bounce) b.reserve(kBounceBytes);
    } catch (const std::bad_alloc&) {
        direct();                                     // no pinned memory to be had: the plain way
        return;
    }
    hipStream_t st = c->slots[0].st;
    const size_t nchunk = (bytes + kBounceBytes - 1) / kBounceBytes;
    const unsigned nthr = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    auto chunk_bytes = [&](size_t k) { return std::min(kBounceBytes, bytes - k * kBounceBytes); };
    // bytes [o, o + len) of the device block -> their rows of the caller's array
    auto scatter = [=](const char* b, size_t o, size_t len) {
        while (len > 0) {
            const size_t row = o / run, within = o - row * run;
            const size_t m = std::min(len, run - within);
            memcpy(static_cast<char*>(dst) + row * dpitch + within, b, m);
            b += m; o += m; len -= m;
        }
    };
    HC(hipMemcpyAsync(c->bounce[0], src_dev, chunk_bytes(0), hipMemcpyDeviceToHost, st));
    for (size_t k = 0; k < nchunk; ++k) {
        HC(hipStreamSynchronize(st));                                           // chunk k has landed in bounce[k & 1]
        if (k + 1 < nchunk)
            HC(hipMemcpyAsync(c->bounce[(k + 1) & 1], static_cast<const char*>(src_dev) + (k + 1) * kBounceBytes,
                              chunk_bytes(k + 1), hipMemcpyDeviceToHost, st));
        const size_t cb = chunk_bytes(k), o0 = k * kBounceBytes;
        const char* b = c->bounce[k & 1];
        const size_t per = ((cb + nthr - 1) / nthr + 4095) & ~size_t(4095);
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nthr; ++t) {
            const size_t o = (size_t)t * per;
            if (o >= cb) break;
            const size_t len = std::min(per, cb - o);
            try { pool.emplace_back([=]() { scatter(b + o, o0 + o, len); }); }
            catch (...) { scatter(b + o, o0 + o, len); }        // no thread to be had: copy this slice here
        }
        scatter(b, o0, std::min(per, cb));
        for (auto& th : pool) th.join();
    }
}
void copy_out_large(gpslc_ctx* c, void* dst, const void* src_dev, size_t bytes) { copy_out_rows(c, dst, bytes, src_dev, bytes, 1); }

// The gradient outputs of gpslc_nodes_logpdf_grad (host, any may be null): dF and dls are the nodes' n x nF_i blocks and nF_i
// values concatenated in node order, dscale and dnoise hold `count` values, dtarget is n x count
struct NodeGradOut {
    double *dF, *dls, *dscale, *dnoise, *dtarget;
    bool any() const { return dF || dls || dscale || dnoise || dtarget; }
};

// scores `count` nodes in ONE launch; logdet/quad/info per node come back through the pinned buffer.
// Returns the first failing pivot (0 = all fine); logpdf[i] = gauss_logpdf(n, logdet_i, quad_i).
// draw_out (optional, host, n x count): node i also returns chol(K_i) * target_i.
// grad (optional; RBF nodes that fit small_grad_lds_bytes): the same launch also differentiates every score (k_small.hip); a
// node whose factorisation broke down gets NaN.
int small_nodes_logpdf(gpslc_ctx* c, int count, const HostNode* nodes, double* logpdf, double* draw_out = nullptr,
                       const NodeGradOut* grad = nullptr) {
    ensure_streams(c);
    const size_t n = (size_t)c->n;
    auto stage = [&](int i) { return NodeStage(n, (size_t)nodes[i].nF, grad != nullptr); };     // sm_layout.h
    size_t doubles = 0, gdoubles = 0;
    int nF_max = 0;
    for (int i = 0; i < count; ++i) {
        doubles += stage(i).in_total; gdoubles += stage(i).out_total;
        nF_max = std::max(nF_max, nodes[i].nF);
    }
    const size_t off_out = ((size_t)count * sizeof(SmallNode) + 63) & ~size_t(63);
    const size_t off_data = off_out + NodeStage::header((size_t)count) * sizeof(double);
    const size_t off_draw = off_data + doubles * sizeof(double);          // [count][n] draws (pinned, written by the kernel)
    const size_t off_grad = off_draw + (draw_out ? (size_t)count * n * sizeof(double) : 0);     // the gradient launch's result block
    c->pin.reserve((off_grad + gdoubles * sizeof(double) + 4095) & ~size_t(4095));
    void* dbase = nullptr;
    HC(hipHostGetDevicePointer(&dbase, c->pin, 0));
    char* dev = static_cast<char*>(dbase);
    SmallNode* hn = c->pin.as<SmallNode>();
    double* hout = reinterpret_cast<double*>(c->pin + off_out);
    double* hd = reinterpret_cast<double*>(c->pin + off_data);
    double* dd = reinterpret_cast<double*>(dev + off_data);
    size_t o = 0, go = 0;        // where node i's input and results start
    for (int i = 0; i < count; ++i) {
        const HostNode& h = nodes[i];
        const NodeStage S = stage(i);
        SmallNode& sn = hn[i];
        sn.nF = h.nF; sn.gofs = (int)go; sn.scale = h.scale; sn.noise = h.noise;
        sn.cov = h.dev_cov; sn.covscale = h.covscale;
        sn.Fs = dd + o;
        sn.target = dd + o + S.target;
        // a feature column goes in twice: divided by its lengthscale, x * (1 / l), the arithmetic of the general path, and
        // (gradient) as it is with the lengthscale, because D comes from the raw features
        size_t f = 0;
        auto put = [&](const double* col, double l) {
            const double il = 1.0 / l;
            for (size_t r = 0; r < n; ++r) hd[o + f * n + r] = col[r] * il;
            if (grad) { memcpy(hd + o + S.raw + f * n, col, n * sizeof(double)); hd[o + S.ls + f] = l; }
            ++f;
        };
        for (int g = 0; g < 2; ++g)
            for (int k = 0; k < h.nFpart[g]; ++k) put(h.F[g] + (size_t)k * n, h.ls[g][k]);
        if (h.col) put(h.col, h.ls_col);
        memcpy(hd + o + S.target, h.target, n * sizeof(double));
        o += S.in_total; go += S.out_total;
    }
    SmallArgs a{};
    a.nodes = reinterpret_cast<const SmallNode*>(dev);
    for (int i = 0; i < std::min(count, SMALL_INLINE_NODES); ++i) a.inl[i] = hn[i];
    a.n = (int)n; a.NB = (int)((n + 15) / 16);
    a.out = reinterpret_cast<double*>(dev + off_out);
    a.draw = draw_out ? reinterpret_cast<double*>(dev + off_draw) : nullptr;
    const bool in_lds = grad || small_gp_lds_bytes((int)n, nF_max) <= kLdsCapBytes;
    if (grad && small_grad_lds_bytes((int)n, nF_max) > kLdsCapBytes) throw std::runtime_error("gradient launch beyond its LDS image");
    if (!in_lds) {       // mid-size kernel: per-node scratch for the finished block columns and the scaled features
        const size_t per = (mid_gp_scratch_doubles((int)n, nF_max) + 31) & ~size_t(31);
        c->scratch.reserve(per * (size_t)count * sizeof(double) + 256);
        c->scratch.reset();
        a.scratch = c->scratch.take<double>(per * (size_t)count);
        a.scratch_stride = (long long)per;
    }
#ifdef GPSLC_DIAG
    static const int want_stamps = diag_env("GPSLC_SMALL_STAMPS", 0);
    if (want_stamps) a.stamps = a.out + NodeStage::kResult * (size_t)count;
#endif
    hipStream_t st = c->slots[0].st;
    if (grad) launch_small_grad(a, reinterpret_cast<double*>(dev + off_grad), count, nF_max, st);
    else if (in_lds) launch_small_gp(a, count, nF_max, st);
    else launch_mid_gp(a, count, nF_max, st);
    HC(hipGetLastError());
    HC(hipStreamSynchronize(st));
#ifdef GPSLC_DIAG
    if (want_stamps && in_lds) {
        static int printed = 0;
        const double* sp = hout + NodeStage::kResult * (size_t)count;
        if (printed++ < want_stamps)
            fprintf(stderr, "small_gp stamps (shader clocks): inputs %.0f gram %.0f factor+panel %.0f (wave 0 inside the pivot chains: %.0f) update %.0f total %.0f\n",
                    sp[0], sp[1], sp[2], sp[4], sp[3], sp[5]);
    }
    if (want_stamps && !in_lds) {      // node 0, per wave: cumulative shader clocks of the phases over all block columns
        static int printed = 0;
        const double* sp = hout + (NodeStage::kResult + NodeStage::kStamps) * (size_t)count;
        if (printed++ < want_stamps)
            for (int w = 0; w < kSmWaves; ++w, sp += NodeStage::kWaveStamps / kSmWaves)
                fprintf(stderr, "mid_gp wave %d: gram %.0f k-loop %.0f to-LDS %.0f wait %.0f factor+store %.0f wait %.0f\n", w,
                        sp[0], sp[1], sp[2], sp[3], sp[4], sp[5]);
    }
#endif
    if (draw_out) memcpy(draw_out, c->pin + off_draw, (size_t)count * n * sizeof(double));
    int first = 0;
    c->last_info.resize((size_t)count);
    for (int i = 0; i < count; ++i) {
        const double* res = hout + NodeStage::kResult * (size_t)i;        // logdet, quad, info
        const int info = (int)res[2];
        c->last_info[i] = info;
        if (info != 0 && first == 0) first = info;
        logpdf[i] = gauss_logpdf(n, res[0], res[1]);
    }
    if (grad) {
        const double* r = reinterpret_cast<const double*>(c->pin + off_grad);
        size_t fo = 0, lo = 0;        // node i's slots of dF and dls
        auto deliver = [](double* dst, const double* src, size_t cnt, bool bad) {
            if (!dst) return;
            if (bad) std::fill(dst, dst + cnt, (double)NAN);
            else memcpy(dst, src, cnt * sizeof(double));
        };
        for (int i = 0; i < count; ++i) {
            const NodeStage S = stage(i);
            const size_t nF = (size_t)nodes[i].nF;
            const bool bad = c->last_info[i] != 0;
            deliver(grad->dF ? grad->dF + fo : nullptr, r, n * nF, bad);
            deliver(grad->dls ? grad->dls + lo : nullptr, r + S.dls, nF, bad);
            deliver(grad->dscale ? grad->dscale + i : nullptr, r + S.dscale, 1, bad);
            deliver(grad->dnoise ? grad->dnoise + i : nullptr, r + S.dnoise, 1, bad);
            deliver(grad->dtarget ? grad->dtarget + (size_t)i * n : nullptr, r + S.dtarget, n, bad);
            fo += n * nF; lo += nF; r += S.out_total;
        }
    }
    return first;
}

}  // namespace

extern "C" {

const char* gpslc_version(void) { return "gpslc_hip 0.1 gfx950"; }

int gpslc_create(gpslc_ctx** out, int device, int64_t n, int32_t nX, int32_t nU, uint32_t flags) {
    if (!out) return -1;
    *out = nullptr;
    if (n < 1) return -3;
    if (nX < 0) return -4;
    if (nU < 0) return -5;
    if (nX + nU > 32) return -4;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return GPSLC_ERR_NODEVICE; }
    if (device < 0 || device >= ndev) return -2;
    gpslc_ctx* c = new (std::nothrow) gpslc_ctx();
    if (!c) return GPSLC_ERR_NOMEM;
    c->device = device; c->n = n; c->nX = nX; c->nU = nU; c->flags = flags;
    c->nt = (int)((n + GP_TS - 1) / GP_TS);
    int rc = guarded(c, [&]() {
        hipDeviceProp_t prop;
        HC(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            set_err(c, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
            return GPSLC_ERR_NODEVICE;
        }
        c->dX.reserve(sizeof(double) * std::max<int64_t>(1, n * nX));
        c->dT.reserve(sizeof(double) * n);
        c->dY.reserve(sizeof(double) * n);
        // defined contents before gpslc_set_data: the node-score entry points that bring their own features and
        // target (gpslc_gp_logpdf, gpslc_mvn_logpdf) work on a ctx without data
        HC(hipMemset(c->dX, 0, sizeof(double) * std::max<int64_t>(1, n * nX)));
        HC(hipMemset(c->dT, 0, sizeof(double) * n));
        HC(hipMemset(c->dY, 0, sizeof(double) * n));
        ensure_streams(c);
        return GPSLC_OK;
    });
    if (rc != GPSLC_OK) { gpslc_destroy(c); return rc; }
    *out = c;
    return GPSLC_OK;
}

int gpslc_destroy(gpslc_ctx* c) {
    if (!c) return GPSLC_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
    return GPSLC_OK;
}

static int set_data_impl(gpslc_ctx* c, const double* X, const double* T, const double* Y, hipMemcpyKind kind) {
    if (!c) return -1;
    if (c->nX > 0 && !X) return bad_arg(c, 2, "X is NULL but nX > 0");
    if (!T) return bad_arg(c, 3, "T is NULL");
    if (!Y) return bad_arg(c, 4, "Y is NULL");
    return guarded(c, [&]() {
        if (c->nX > 0) HC(hipMemcpy(c->dX, X, sizeof(double) * c->n * c->nX, kind));
        HC(hipMemcpy(c->dT, T, sizeof(double) * c->n, kind));
        HC(hipMemcpy(c->dY, Y, sizeof(double) * c->n, kind));
        c->hX.resize((size_t)c->n * c->nX);
        c->hT.resize(c->n);
        c->hY.resize(c->n);
        if (c->nX > 0) HC(hipMemcpy(c->hX.data(), c->dX, sizeof(double) * c->n * c->nX, hipMemcpyDeviceToHost));
        HC(hipMemcpy(c->hT.data(), c->dT, sizeof(double) * c->n, hipMemcpyDeviceToHost));
        HC(hipMemcpy(c->hY.data(), c->dY, sizeof(double) * c->n, hipMemcpyDeviceToHost));
        c->binary_t = true;
        for (double t : c->hT) if (t != 0.0 && t != 1.0) { c->binary_t = false; break; }
        c->has_data = true;
        c->ens_off = 0; c->ens_S = 0;      // a new data set starts outside any ensemble placement
        return GPSLC_OK;
    });
}
int gpslc_set_data(gpslc_ctx* c, const double* X, const double* T, const double* Y) {
    return set_data_impl(c, X, T, Y, hipMemcpyHostToDevice);
}
int gpslc_set_data_dev(gpslc_ctx* c, const double* X, const double* T, const double* Y) {
    return set_data_impl(c, X, T, Y, hipMemcpyDeviceToDevice);
}

int gpslc_set_tuning(gpslc_ctx* c, int32_t max_batch, int32_t panel_tiles, int32_t n_streams) {
    if (!c) return -1;
    if (max_batch < 0) return -2;
    if (panel_tiles < 0) return -3;
    if (n_streams < 0 || n_streams > 8) return -4;
    if (max_batch > 0) c->max_batch = max_batch;
    if (panel_tiles > 0) { c->panel = panel_tiles; c->panel_set = true; }
    if (n_streams > 0) c->nstreams = n_streams;
    return GPSLC_OK;
}

int gpslc_set_task_schedule(gpslc_ctx* c, int32_t min_tiles, int32_t max_tiles, int32_t min_matrices, int32_t group) {
    if (!c) return -1;
    if (min_tiles > TASK_MAX_NT) return -2;
    if (max_tiles > TASK_MAX_NT) return -3;
    if (group > 4096) return -5;
    if (min_tiles > 0) c->task_min_nt = min_tiles;
    if (max_tiles >= 0) c->task_max_nt = max_tiles;
    if (min_matrices > 0) c->task_min_batch = min_matrices;
    if (group > 0) c->task_group = group;
    return GPSLC_OK;
}

const char* gpslc_last_error(const gpslc_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gpslc_set_ensemble(gpslc_ctx* c, int64_t sample_offset, int64_t S_total) {
    if (!c) return -1;
    if (sample_offset < 0) return -2;
    if (S_total < 0 || (S_total > 0 && sample_offset >= S_total)) return -3;
    c->ens_off = S_total > 0 ? sample_offset : 0;
    c->ens_S = S_total;
    return 0;
}

static int rbf_log_check(gpslc_ctx* c, const double* X1, const double* X2, int64_t n, int32_t d, const double* ls,
                         int32_t ls_len, double* out) {
    if (!c) return -1;
    if (!X1) return bad_arg(c, 2, "X1 is NULL");
    if (!X2) return bad_arg(c, 3, "X2 is NULL");
    if (n < 1) return bad_arg(c, 4, "n < 1");
    if (d < 1) return bad_arg(c, 5, "d < 1");
    if (!ls) return bad_arg(c, 6, "ls is NULL");
    if (ls_len != 1 && ls_len != d) return bad_arg(c, 7, "vector lengthscale doesn't match individual");
    if (!out) return bad_arg(c, 8, "out is NULL");
    return 0;
}

int gpslc_rbf_log_dev(gpslc_ctx* c, const double* X1, const double* X2, int64_t n, int32_t d, const double* ls,
                      int32_t ls_len, double* out) {
    int rc = rbf_log_check(c, X1, X2, n, d, ls, ls_len, out);
    if (rc) return rc;
    return guarded(c, [&]() {
        ensure_streams(c);
        launch_rbf_log(X1, X2, n, d, ls, ls_len, out, c->slots[0].st);
        HC(hipGetLastError());
        HC(hipStreamSynchronize(c->slots[0].st));
        return GPSLC_OK;
    });
}

// the host forms: upload, run what the _dev form runs, copy out

int gpslc_rbf_log(gpslc_ctx* c, const double* X1, const double* X2, int64_t n, int32_t d, const double* ls,
                  int32_t ls_len, double* out) {
    int rc = rbf_log_check(c, X1, X2, n, d, ls, ls_len, out);
    if (rc) return rc;
    return guarded(c, [&]() {
        c->io.reset();
        double* dA = up(c, X1, (size_t)n * d);
        double* dB = up(c, X2, (size_t)n * d);
        double* dl = up(c, ls, (size_t)ls_len);
        double* o = c->io.take<double>((size_t)n * n);
        const int st = gpslc_rbf_log_dev(c, dA, dB, n, d, dl, ls_len, o);
        if (st == GPSLC_OK) copy_out_large(c, out, o, sizeof(double) * (size_t)n * n);
        return st;
    });
}

int gpslc_process_cov_dev(gpslc_ctx* c, const double* logcov, int64_t n, double scale, double noise, double* out) {
    if (!c) return -1;
    if (!logcov) return bad_arg(c, 2, "logcov is NULL");
    if (n < 1) return bad_arg(c, 3, "n < 1");
    if (!out) return bad_arg(c, 6, "out is NULL");
    return guarded(c, [&]() {
        ensure_streams(c);
        launch_process_cov(logcov, n, scale, noise, out, c->slots[0].st);
        HC(hipGetLastError());
        HC(hipStreamSynchronize(c->slots[0].st));
        return GPSLC_OK;
    });
}

int gpslc_process_cov(gpslc_ctx* c, const double* logcov, int64_t n, double scale, double noise, double* out) {
    if (!c) return -1;
    if (!logcov) return bad_arg(c, 2, "logcov is NULL");
    if (n < 1) return bad_arg(c, 3, "n < 1");
    if (!out) return bad_arg(c, 6, "out is NULL");
    return guarded(c, [&]() {
        c->io.reset();
        double* dA = up(c, logcov, (size_t)n * n);
        double* o = c->io.take<double>((size_t)n * n);
        const int st = gpslc_process_cov_dev(c, dA, n, scale, noise, o);
        if (st == GPSLC_OK) copy_out_large(c, out, o, sizeof(double) * (size_t)n * n);
        return st;
    });
}

// Where a host-pointer prediction over the samples [s0, s0 + S) of S_total sits in the caller's arrays (gpslc_predict_multi:
// one shard; gpslc_predict: s0 = 0, S_total = S).  Per-sample inputs and the outputs are addressed in the caller's FULL
// arrays: element (s, l) of an S_total x L array at (s0 + s) + S_total l, block (s, l) of an n x S_total x L array at
// n ((s0 + s) + S_total l); the level-fastest draw tensor keeps a shard's columns contiguous.
struct HostPlacement {
    int64_t s0 = 0, S_total = 0;
    int64_t ens_off = 0, ens_S = 0;     // Philox stream placement of the shard (ens_S > 0), else the ctx's
};

// what an extern "C" prediction or ITE-distribution function was asked for, with the caller's pointers as given
struct PredictRequest {
    Posterior post;
    Levels lv;
    DrawsAndOutputs out;
    double *MeanITEs = nullptr, *CovITEs = nullptr;     // gpslc_ite_distributions*: S x n, S x n x n
    HostPlacement pl;                                   // host calls
};
static PredictRequest make_request(int64_t S, const SampleParams& samples, int32_t L, const double* doT) {
    PredictRequest rq;
    rq.post.S = S; rq.post.p = samples;
    rq.lv.L = L; rq.lv.doT = doT;
    rq.pl.S_total = S;
    return rq;
}

// The position of each checked argument in one entry point's signature (0: it has no such argument): the k of the status -k
// and of the message's "argument #k".  fp64_only: the entry point refuses a GPSLC_FLAG_FP32_KERNEL context (the fp32 kernel
// mode covers scalar levels without baseline or weights only).
// covW: the joint covariance where the weights are optional (it needs them).
struct ArgPos { int S, U, xyLS, tyLS, L, doT, base, G, W, spp; bool fp64_only; int covW = 0; };
static const ArgPos kPredictArgs{2, 3, 5, 6, 9, 10, 0, 0, 0, 12, false}, kPredictVecArgs{2, 3, 5, 6, 9, 10, 0, 0, 0, 12, true},
    kPredictContrastArgs{2, 3, 5, 6, 9, 10, 11, 0, 0, 13, true}, kPredictWeightedArgs{2, 3, 5, 6, 9, 10, 11, 12, 13, 15, true},
    kPredictMultiArgs{3, 4, 6, 7, 10, 11, 0, 0, 0, 13, false},      // two more leading arguments: nctx, ctxs
    kSamplesArgs{2, 3, 5, 6, 0, 0, 0, 0, 0, 0, false},      // gpslc_ite_distributions, gpslc_y_logpdf, gpslc_y_loo, gpslc_y_lgo, gpslc_likelihood_distribution
    kIteVecArgs{2, 3, 5, 6, 0, 9, 0, 0, 0, 0, true}, kIteContrastArgs{2, 3, 5, 6, 0, 9, 10, 0, 0, 0, true},
    kLikelihoodVecArgs{2, 3, 5, 6, 0, 8, 0, 0, 0, 0, false},
    kPredictSlopeArgs{2, 3, 5, 6, 9, 10, 0, 11, 12, 14, true, 19}, kIteSlopeArgs{2, 3, 5, 6, 0, 9, 0, 0, 0, 0, true};
// the outcome entry points share their twins' positions: gpslc_predict_outcome kPredictSlopeArgs, gpslc_predict_outcome_vec
// kPredictVecArgs, gpslc_ite_distributions_outcome kIteSlopeArgs, gpslc_ite_distributions_outcome_vec kIteVecArgs

// `count` host values: all there and all finite
static int finite_check(gpslc_ctx* c, const double* v, int64_t count, int argk, const char* name) {
    char what[64];
    if (!v) { snprintf(what, sizeof what, "%s is NULL", name); return bad_arg(c, argk, what); }
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) { snprintf(what, sizeof what, "%s has a non-finite entry", name); return bad_arg(c, argk, what); }
    return 0;
}

// The argument checks of every prediction and ITE-distribution entry point, in the order of the arguments.  Levels given as
// host values beyond the plain L scalars (vector levels: n x L; pairs with a baseline; slopes; outcomes; weight columns: n x G) must
// be finite.  The slope and outcome entries take their weights or none (G == 0 and NULL: the plain 1/n average).
static int validate(gpslc_ctx* c, const PredictRequest& rq, const ArgPos& k) {
    const Posterior& po = rq.post;
    const Levels& lv = rq.lv;
    if (!c) return -1;
    if (!c->has_data) { set_err(c, "gpslc_set_data has not been called"); return GPSLC_ERR_NODATA; }
    if (po.S < 0) return bad_arg(c, k.S, "S < 0");
    if (c->nU > 0 && po.S > 0 && (!po.p.U || !po.p.uyLS)) return bad_arg(c, k.U, "U / uyLS must not be NULL when nU > 0");
    if (c->nX > 0 && po.S > 0 && !po.p.xyLS) return bad_arg(c, k.xyLS, "xyLS must not be NULL when nX > 0");
    if (po.S > 0 && (!po.p.tyLS || !po.p.yScale || !po.p.yNoise)) return bad_arg(c, k.tyLS, "tyLS / yScale / yNoise must not be NULL");
    const bool no_spp = rq.out.ite_draws && rq.out.spp < 1;
    int rc = 0;
    if (k.L) {
        if (lv.L < 1) return bad_arg(c, k.L, "L < 1");
        if (!lv.doT) return bad_arg(c, k.doT, "doT is NULL");
        if (no_spp && !k.base && !k.W) return bad_arg(c, k.spp, "spp < 1 with ite_draws requested");      // spp follows doT
        // a placement left over from an earlier, smaller call would make the stream ids (off + s) + S_total * l of this call's
        // last samples collide with the next level's streams: refuse instead of drawing correlated normals
        if (c->ens_S > 0 && c->ens_off + po.S > c->ens_S)
            return bad_arg(c, k.S, "S exceeds the room gpslc_set_ensemble left: sample_offset + S > S_total");
    }
    if (lv.vec || k.base || lv.form == FORM_SLOPE || lv.form == FORM_OUTCOME) {
        if ((rc = finite_check(c, lv.doT, lv.vec ? c->n * (int64_t)lv.L : lv.L, k.doT, "doT"))) return rc;
        // the baselines are optional beside weights
        if (k.base && (lv.base || !k.W) && (rc = finite_check(c, lv.base, lv.L, k.base, "doT_base"))) return rc;
    }
    if (k.W && k.covW) {       // optional weights
        if (lv.G < 0) return bad_arg(c, k.G, "G < 0");
        if (lv.G == 0 && lv.W) return bad_arg(c, k.G, "G == 0 with weights given");
        if (lv.G > 0 && (rc = finite_check(c, lv.W, c->n * (int64_t)lv.G, k.W, "weights"))) return rc;
    } else if (k.W) {
        if (lv.G < 1) return bad_arg(c, k.G, "G < 1");
        if ((rc = finite_check(c, lv.W, c->n * (int64_t)lv.G, k.W, "weights"))) return rc;
    }
    if (no_spp && (k.base || k.W)) return bad_arg(c, k.spp, "spp < 1 with ite_draws requested");
    if (k.covW && rq.out.covW && !lv.W) return bad_arg(c, k.covW, "covW needs weights");
    if (k.fp64_only && (c->flags & GPSLC_FLAG_FP32_KERNEL)) {
        set_err(c, "vector levels, contrasts, slopes, outcomes and weighted effects are not supported on a GPSLC_FLAG_FP32_KERNEL context (fp64 only)");
        return GPSLC_ERR_UNSUPPORTED;
    }
    return 0;
}

// the samples [s0, s0 + S) of a host posterior block, uploaded into the staging pool
static SampleParams upload_samples(gpslc_ctx* c, const SampleParams& h, size_t s0, size_t S) {
    const size_t n = (size_t)c->n, nU = (size_t)c->nU, nX = (size_t)c->nX;
    SampleParams d{};
    d.U = nU ? up(c, h.U + n * nU * s0, n * nU * S) : nullptr;
    d.uyLS = nU ? up(c, h.uyLS + nU * s0, nU * S) : nullptr;
    d.xyLS = nX ? up(c, h.xyLS + nX * s0, nX * S) : nullptr;
    d.tyLS = up(c, h.tyLS + s0, S);
    d.yScale = up(c, h.yScale + s0, S);
    d.yNoise = up(c, h.yNoise + s0, S);
    return d;
}

// device pointers everywhere; the info words come from the staging pool (the caller has reset it)
static int predict_dev_inner(gpslc_ctx* c, const PredictRequest& rq) {
    PredictIO io;
    io.post = rq.post; io.lv = rq.lv; io.out = rq.out; io.X = c->dX;
    io.MeanITEs = rq.MeanITEs; io.CovITEs = rq.CovITEs;
    io.ens_off = rq.pl.ens_off; io.ens_S = rq.pl.ens_S;
    io.info = c->io.take<int>((size_t)rq.post.S);
    run_predict(c, io);
    return first_info(c);
}

int gpslc_predict_dev(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                      const double* tyLS, const double* yScale, const double* yNoise, int32_t L,
                      const double* doT, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                      double* meanSATE, double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictArgs);
    if (rc) return rc;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        c->io.reset();
        return predict_dev_inner(c, rq);
    });
}

// The body of the host-pointer entry points (an empty call returns here, after its checks): uploads, run_predict, delivery —
// every level's run of a shard goes from the device straight to its place in the caller's array (no host staging, VERDICT r05
// item 2)
static int predict_host(gpslc_ctx* c, const PredictRequest& rq) {
    const int64_t S = rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const Levels& lv = rq.lv;
        const DrawsAndOutputs& o = rq.out;
        const size_t n = (size_t)c->n, L = (size_t)lv.L;
        const size_t LR = lv.W ? L * lv.G : L;     // meanSATE / varSATE columns: levels, or levels x weight columns
        const size_t s0 = (size_t)rq.pl.s0, St = (size_t)rq.pl.S_total;
        c->io.reset();
        PredictRequest d = rq;             // the same request with device pointers
        d.post.p = upload_samples(c, rq.post.p, s0, (size_t)S);
        d.lv.doT = up(c, lv.doT, lv.vec ? n * L : L);                 // vector levels: n x L
        d.lv.base = lv.base ? up(c, lv.base, L) : nullptr;            // contrasts: the L baselines
        if (lv.W) {                // n x G host (weights[i + n*g]) -> column fastest on the device (W[g + G*i]: the kernels' layout)
            const size_t G = (size_t)lv.G;
            std::vector<double> wt(n * G);
            for (size_t i = 0; i < n; ++i)
                for (size_t g = 0; g < G; ++g) wt[g + G * i] = lv.W[i + n * g];
            d.lv.W = up(c, wt.data(), wt.size());
        }
        d.out.z = nullptr;
        if (o.z && o.ite_draws) {  // caller's normals n x spp x S_total x L: level l of the shard is one run of n spp S doubles
            double* dz = c->io.take<double>(n * o.spp * S * L);
            const size_t run = n * o.spp * (size_t)S * sizeof(double);
            HC(hipMemcpy2D(dz, run, o.z + n * o.spp * s0, n * o.spp * St * sizeof(double), run, L, hipMemcpyHostToDevice));
            d.out.z = dz;
        }
        double* oms = d.out.meanSATE = o.meanSATE ? c->io.take<double>((size_t)S * LR) : nullptr;
        // the joint covariance takes its diagonal from the device's varW, asked for or not
        double* ovs = d.out.varSATE = (o.varSATE || o.covW) ? c->io.take<double>((size_t)S * LR) : nullptr;
        double* ocv = d.out.covW = o.covW ? c->io.take<double>((size_t)S * LR * L) : nullptr;
        double* omi = d.out.meanITE = o.meanITE ? c->io.take<double>(n * S * L) : nullptr;
        double* odr = d.out.ite_draws = o.ite_draws ? c->io.take<double>(L * n * S * o.spp) : nullptr;
        int st = predict_dev_inner(c, d);
        if (st < 0) return st;
        const size_t sb = (size_t)S * sizeof(double);
        if (o.meanSATE) HC(hipMemcpy2D(o.meanSATE + s0, St * sizeof(double), oms, sb, sb, LR, hipMemcpyDeviceToHost));
        if (o.varSATE) HC(hipMemcpy2D(o.varSATE + s0, St * sizeof(double), ovs, sb, sb, LR, hipMemcpyDeviceToHost));
        if (o.covW) copy_out_rows(c, o.covW + s0, St * sizeof(double), ocv, sb, LR * L);
        if (o.meanITE) copy_out_rows(c, o.meanITE + n * s0, n * St * sizeof(double), omi, n * sb, L);
        // level-fastest tensor L x n x (S_total spp): a sample's columns are one contiguous run
        if (o.ite_draws) copy_out_large(c, o.ite_draws + L * n * o.spp * s0, odr, sizeof(double) * L * n * S * o.spp);
        return st;
    });
}

int gpslc_predict(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                  const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                  double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                  double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictArgs);
    return rc ? rc : predict_host(c, rq);
}

// vector levels: every entry of the n x L host array doT must be finite
int gpslc_predict_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                      const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                      double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                      double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.vec = true;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictVecArgs);
    return rc ? rc : predict_host(c, rq);
}

// contrasts: level l is the pair (doT[l], doT_base[l]) of finite scalars
int gpslc_predict_contrast(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                           const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                           const double* doT_base, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                           double* meanSATE, double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictContrastArgs);
    return rc ? rc : predict_host(c, rq);
}

// weighted effects: G >= 1 columns of n finite host weights each; scalar levels, with or without baselines
int gpslc_predict_weighted(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                           const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                           const double* doT_base, int32_t G, const double* weights, double pred_noise, int32_t spp,
                           uint64_t seed, const double* z, double* meanW, double* varW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base); rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictWeightedArgs);
    return rc ? rc : predict_host(c, rq);
}

// the same call with the joint covariance of the levels per weight column as one more output
int gpslc_predict_curve(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                        const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                        const double* doT_base, int32_t G, const double* weights, double pred_noise, int32_t spp,
                        uint64_t seed, const double* z, double* meanW, double* varW, double* covW, double* meanITE,
                        double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.against(doT_base); rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictWeightedArgs);
    return rc ? rc : predict_host(c, rq);
}

// marginal effects: level l is the slope d f_i(t) / dt at the finite scalar t = doT[l].  G == 0 and NULL weights:
// the plain 1/n average as gpslc_predict's (covW must be NULL); else G >= 1 weight columns as gpslc_predict_curve's
int gpslc_predict_slope(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                        const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                        int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                        double* meanW, double* varW, double* covW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.form = FORM_SLOPE; rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictSlopeArgs);
    return rc ? rc : predict_host(c, rq);
}

// potential outcomes: level l is f_i(doT[l]) itself, everybody set to the finite scalar doT[l].  Arguments, weights
// (or none) and checks are gpslc_predict_slope's
int gpslc_predict_outcome(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                          const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                          int32_t G, const double* weights, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                          double* meanW, double* varW, double* covW, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.form = FORM_OUTCOME; rq.lv.G = G; rq.lv.W = weights;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanW, varW, meanITE, ite_draws, covW};
    int rc = validate(c, rq, kPredictSlopeArgs);
    return rc ? rc : predict_host(c, rq);
}

// the outcome at vector levels: individual i set to doT[i + n*l]; arguments and checks are gpslc_predict_vec's
int gpslc_predict_outcome_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                              const double* tyLS, const double* yScale, const double* yNoise, int32_t L, const double* doT,
                              double pred_noise, int32_t spp, uint64_t seed, const double* z, double* meanSATE,
                              double* varSATE, double* meanITE, double* ite_draws) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.lv.vec = true; rq.lv.form = FORM_OUTCOME;
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc = validate(c, rq, kPredictVecArgs);
    return rc ? rc : predict_host(c, rq);
}

int gpslc_shard_range(int64_t S, int32_t nblocks, int32_t k, int64_t* s0, int64_t* s1) {
    if (S < 0) return -1;
    if (nblocks < 1) return -2;
    if (k < 0 || k >= nblocks) return -3;
    if (!s0) return -4;
    if (!s1) return -5;
    const int64_t q = S / nblocks, r = S % nblocks;
    *s0 = k * q + std::min<int64_t>(k, r);
    *s1 = *s0 + q + (k < r ? 1 : 0);
    return GPSLC_OK;
}

// The sharded ensemble behind the ABI (the loop src/prediction.jl:30-33 over src/estimation.jl:78-84): contiguous
// blocks of the posterior-sample index over the contexts, one host thread per context, data replicated (every ctx holds its own
// copy: gpslc_set_data), no traffic between the devices while they compute.  The "gather" is each device's own device-to-host
// copy into ITS block of the caller's arrays — nctx PCIe links in parallel, nothing funnels through one GPU — and since round 6
// every level's run of a shard goes from the device (through the ctx's pinned bounce chunks) straight to its place in the
// caller's array: no per-shard host staging, no second pass over the results.  A shard's ensemble placement travels as a
// parameter: the contexts' own gpslc_set_ensemble state is read (ctxs[0]'s places the whole call), never written.
int gpslc_predict_multi(int32_t nctx, gpslc_ctx* const* ctxs, int64_t S, const double* U, const double* uyLS,
                        const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise, int32_t L,
                        const double* doT, double pred_noise, int32_t spp, uint64_t seed, const double* z,
                        double* meanSATE, double* varSATE, double* meanITE, double* ite_draws, int32_t* info_or_null) {
    if (nctx < 1) return -1;
    if (!ctxs) return -2;
    for (int k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return -2;
        for (int j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return bad_arg(ctxs[0], 2, "the same ctx is listed twice (one ctx per shard: calls on a ctx are serialised)");
    }
    gpslc_ctx* c0 = ctxs[0];
    for (int k = 1; k < nctx; ++k) {
        if (ctxs[k]->n != c0->n || ctxs[k]->nX != c0->nX || ctxs[k]->nU != c0->nU)
            return bad_arg(c0, 2, "the contexts differ in n / nX / nU");
        // one precision mode per call: a ctx created with GPSLC_FLAG_FP32_KERNEL would silently mix arithmetics across the shards
        if ((ctxs[k]->flags & GPSLC_FLAG_FP32_KERNEL) != (c0->flags & GPSLC_FLAG_FP32_KERNEL))
            return bad_arg(c0, 2, "the contexts differ in GPSLC_FLAG_FP32_KERNEL");
        if (!ctxs[k]->has_data) { set_err(c0, "gpslc_set_data has not been called on every ctx"); return GPSLC_ERR_NODATA; }
    }
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    rq.out = DrawsAndOutputs{pred_noise, spp, seed, z, meanSATE, varSATE, meanITE, ite_draws};
    int rc0 = validate(c0, rq, kPredictMultiArgs);      // argument numbers of THIS signature, in the code and in the message
    if (rc0) return rc0;
    if (S == 0) { for (int k = 0; k < nctx; ++k) ctxs[k]->last_info.clear(); return GPSLC_OK; }
    try {
        // placement of the whole call (ctxs[0]'s, if the caller set one: this call may itself be one node's share)
        const int64_t base_off = c0->ens_S > 0 ? c0->ens_off : 0, total = c0->ens_S > 0 ? c0->ens_S : S;
        struct Shard { int64_t s0 = 0, Sr = 0; int rc = 0; };
        std::vector<Shard> sh((size_t)nctx);
        for (int k = 0; k < nctx; ++k) {
            int64_t s1 = 0;
            (void)gpslc_shard_range(S, nctx, k, &sh[(size_t)k].s0, &s1);
            sh[(size_t)k].Sr = s1 - sh[(size_t)k].s0;
        }
        auto work = [&](int k) {
            Shard& h = sh[(size_t)k];
            if (h.Sr == 0) { ctxs[k]->last_info.clear(); return; }
            PredictRequest part = rq;                // the shard's samples, placed in the caller's full arrays
            part.post.S = h.Sr;
            part.pl = HostPlacement{h.s0, S, base_off + h.s0, total};
            h.rc = predict_host(ctxs[k], part);
        };
        std::vector<std::thread> pool;
        for (int k = 1; k < nctx; ++k) {
            try { pool.emplace_back(work, k); }
            catch (...) { work(k); }                 // no thread to be had: this shard runs here, in turn
        }
        work(0);
        for (auto& t : pool) t.join();
        int rc = 0;
        for (int k = 0; k < nctx && rc == 0; ++k)
            if (sh[(size_t)k].rc < 0) {
                rc = sh[(size_t)k].rc;
                if (k > 0) set_err(c0, "shard " + std::to_string(k) + " (device " + std::to_string(ctxs[k]->device) + "): " + ctxs[k]->err);
            }
        for (int k = 0; k < nctx && rc == 0; ++k) rc = sh[(size_t)k].rc;        // blocks are in sample order: the first failing pivot
        if (info_or_null)
            for (int k = 0; k < nctx; ++k) {
                const Shard& h = sh[(size_t)k];
                if (h.Sr == 0) continue;
                if ((int64_t)ctxs[k]->last_info.size() == h.Sr) memcpy(info_or_null + h.s0, ctxs[k]->last_info.data(), sizeof(int32_t) * h.Sr);
                else for (int64_t j = 0; j < h.Sr; ++j) info_or_null[h.s0 + j] = 0;
            }
        return rc;
    } catch (const std::bad_alloc&) {
        set_err(c0, "host allocation failed");
        return GPSLC_ERR_NOMEM;
    } catch (...) {
        set_err(c0, "internal error");
        return GPSLC_ERR_INTERNAL;
    }
}

// gpslc_ite_distributions*'s body: one level (host) — a scalar, n values (vec), the contrast of two scalars (base), a slope or
// an outcome (scalar or vec)
static int ite_distributions_host(gpslc_ctx* c, const PredictRequest& rq) {
    const int64_t S = rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t n = (size_t)c->n;
        c->io.reset();
        PredictRequest d = rq;             // the same request with device pointers
        d.post.p = upload_samples(c, rq.post.p, 0, (size_t)S);
        d.lv.doT = up(c, rq.lv.doT, rq.lv.vec ? n : 1);
        d.lv.base = rq.lv.base ? up(c, rq.lv.base, 1) : nullptr;
        d.MeanITEs = rq.MeanITEs ? c->io.take<double>((size_t)S * n) : nullptr;
        d.CovITEs = rq.CovITEs ? c->io.take<double>((size_t)S * n * n) : nullptr;
        const int st = predict_dev_inner(c, d);
        if (rq.MeanITEs) HC(hipMemcpy(rq.MeanITEs, d.MeanITEs, sizeof(double) * S * n, hipMemcpyDeviceToHost));
        if (rq.CovITEs) copy_out_large(c, rq.CovITEs, d.CovITEs, sizeof(double) * (size_t)S * n * n);
        return st;
    });
}

int gpslc_ite_distributions(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                            const double* tyLS, const double* yScale, const double* yNoise, double doT,
                            double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kSamplesArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                const double* tyLS, const double* yScale, const double* yNoise, const double* doT,
                                double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, doT);
    rq.lv.vec = true;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteVecArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_contrast(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                     const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                     double doT_base, double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.against(&doT_base);
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteContrastArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_slope(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                  const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                  double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.form = FORM_SLOPE;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteSlopeArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_outcome(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                    const double* tyLS, const double* yScale, const double* yNoise, double doT,
                                    double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, &doT);
    rq.lv.form = FORM_OUTCOME;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteSlopeArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

int gpslc_ite_distributions_outcome_vec(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS,
                                        const double* tyLS, const double* yScale, const double* yNoise, const double* doT,
                                        double pred_noise, double* MeanITEs, double* CovITEs) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 1, doT);
    rq.lv.vec = true; rq.lv.form = FORM_OUTCOME;
    rq.out.pred_noise = pred_noise; rq.MeanITEs = MeanITEs; rq.CovITEs = CovITEs;
    int rc = validate(c, rq, kIteVecArgs);
    return rc ? rc : ite_distributions_host(c, rq);
}

}  // extern "C"

// ---- node scores: the six entry points of the chain's inner loop and what they share --------------------------------
namespace {

// The tiled score of the S parameter sets of `io`: the caller has filled in the samples, the features, the right-hand side
// (the value being scored) and, for gpslc_nodes_draw, the node draw.  This adds "no level, score only", runs the prediction
// pass and turns the epilogue's logdet / quad into log-densities.  Returns the first failing pivot.
int tiled_score(gpslc_ctx* c, PredictIO& io, double* logpdf) {
    const size_t S = (size_t)io.post.S;
    const double zero = 0.0;
    io.lv.L = 0; io.lv.doT = up(c, &zero, 1);
    io.logdet = c->io.take<double>(S); io.quad = c->io.take<double>(S); io.info = c->io.take<int>(S);
    run_predict(c, io);
    std::vector<double> ld(S), q(S);
    HC(hipMemcpy(ld.data(), io.logdet, sizeof(double) * S, hipMemcpyDeviceToHost));
    HC(hipMemcpy(q.data(), io.quad, sizeof(double) * S, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S; ++s) logpdf[s] = gauss_logpdf((size_t)c->n, ld[s], q[s]);
    return first_info(c);
}

// One output of an outcome-model call: the caller's array (null: not asked), the io's device pointer that stands for it, doubles
struct Output { double* host; double** dev; size_t count; };
using Outputs = std::initializer_list<Output>;
void take_outputs(gpslc_ctx* c, Outputs outs) {            // staging memory for the asked outputs
    for (const Output& o : outs)
        if (o.host) *o.dev = c->io.take<double>(o.count);
}
void deliver_outputs(gpslc_ctx* c, Outputs outs) {
    for (const Output& o : outs)
        if (o.host) copy_out_large(c, o.host, *o.dev, o.count * sizeof(double));
}

// The body of the outcome-model entry points that score on the tiled factor (gpslc_y_logpdf beyond the single-workgroup kernels,
// gpslc_y_loo, gpslc_y_lgo, gpslc_y_logpdf_grad), after their checks: uploads the request's samples and the
// overrides (Y_or_null: the value being scored — Gen passes it to logpdf — else the ctx's Y), lets `special` add what only this
// call has, takes device memory for the asked outputs (`outs` points into io) and scores.  Nothing is copied out after a negative status.
int outcome_call(gpslc_ctx* c, const PredictRequest& rq, const double* X_or_null, const double* Y_or_null, double* logpdf_or_null,
                 PredictIO& io, Outputs outs, const std::function<void()>& special = nullptr) {
    const size_t n = (size_t)c->n, S = (size_t)rq.post.S;
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        c->io.reset();
        io.post.S = rq.post.S; io.post.p = upload_samples(c, rq.post.p, 0, S);
        io.X = (X_or_null && c->nX) ? up(c, X_or_null, n * c->nX) : c->dX;
        if (Y_or_null) { io.Y = up(c, Y_or_null, n); io.y_sstride = 0; }
        if (special) special();
        take_outputs(c, outs);
        std::vector<double> lp(logpdf_or_null ? 0 : S);       // the scores are computed either way: kept only when the caller asks
        const int st = tiled_score(c, io, logpdf_or_null ? logpdf_or_null : lp.data());
        if (st >= 0) deliver_outputs(c, outs);
        return st;
    });
}

// general (tiled, multi-launch) path of gpslc_gp_logpdf; arguments already validated
// draws_or_null (host, n x S; needs t_shared == 0): also chol(K_s) target_s — the targets are then standard normals
// grad_or_null (host, the layouts of S sets of nF columns: dF n x nF x S, dls nF x S, dtarget n x S): also the gradient of every
// score, §21's pair pass and finish kernel in node mode (GradArgs::no_t)
int gp_logpdf_general(gpslc_ctx* c, int64_t S, int32_t nF, const double* F, int32_t f_shared, const double* ls,
                      const double* scale, const double* noise, const double* target, int32_t t_shared, double* logpdf,
                      double* draws_or_null = nullptr, const NodeGradOut* grad_or_null = nullptr) {
    const size_t n = (size_t)c->n;
    c->io.reset();
    const double* dF = nF ? up(c, F, n * nF * (f_shared ? 1 : S)) : nullptr;
    const double* dls = nF ? up(c, ls, (size_t)nF * S) : nullptr;
    const double* dsc = up(c, scale, S);
    const double* dno = up(c, noise, S);
    const double* dtg = up(c, target, n * (t_shared ? 1 : S));
    std::vector<double> inf(S, INFINITY);        // tyLS = inf switches the treatment term off: e_ij = exp(-0) = 1
    const double* dty = up(c, inf.data(), S);
    PredictIO io;
    io.post.S = S;
    io.post.p = SampleParams{dF, dls, nullptr, dty, dsc, dno, f_shared ? 0 : (long long)n * nF};
    io.p_shared_u = f_shared != 0;
    io.X = nullptr; io.nU = nF; io.nX = 0;
    io.Y = dtg; io.y_sstride = t_shared ? 0 : (long long)n;
    double* ddraw = nullptr;
    if (draws_or_null) {
        ensure_streams(c);
        ddraw = c->io.take<double>(n * (size_t)S);
        double* zero_mean = c->io.take<double>(n * (size_t)S);
        HC(hipMemsetAsync(zero_mean, 0, n * (size_t)S * sizeof(double), c->slots[0].st));
        HC(hipStreamSynchronize(c->slots[0].st));
        io.nz = dtg; io.nzero = zero_mean; io.ndraw = ddraw;
    }
    NodeGradOut g = grad_or_null ? *grad_or_null : NodeGradOut{};
    if (nF == 0) g.dF = g.dls = nullptr;
    const Outputs outs = {{g.dF, &io.grad.U, n * (size_t)nF * S}, {g.dls, &io.grad.uyLS, (size_t)nF * S}, {g.dscale, &io.grad.yScale, (size_t)S},
                          {g.dnoise, &io.grad.yNoise, (size_t)S}, {g.dtarget, &io.grad.Y, n * (size_t)S}};
    io.grad_no_t = true;
    take_outputs(c, outs);
    const int st = tiled_score(c, io, logpdf);
    if (draws_or_null) HC(hipMemcpy(draws_or_null, ddraw, n * (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    deliver_outputs(c, outs);
    return st;
}

// ONE batched pass of the general tiled path over all nodes of a call (S = count parameter sets with per-set feature blocks
// and per-set targets); draws_or_null: also chol(K_i) target_i per node (gpslc_nodes_draw)
int nodes_general(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, int nF_max, double* logpdf, double* draws_or_null,
                  const NodeGradOut* grad_or_null = nullptr) {
    // Nodes with fewer than nF_max feature columns are padded with zero
    // columns of lengthscale 1: a padding column adds (0 * 1 - 0 * 1)^2 = +0.0 to every squared distance, so a
    // node's Gram matrix — and its score — is bit-identical to the one its own feature count would give.
    // Staging lives in the ctx (this call sits in the MCMC inner loop: no allocation once the buffers have grown),
    // and nodes that all share ONE feature block — the nX `:X => k => :X` nodes, F = U for every k — hand it over once
    // (f_shared) instead of count padded copies.
    const size_t n = (size_t)c->n;
    bool same_f = true;
    for (int i = 1; i < count; ++i) same_f = same_f && nodes[i].F == nodes[0].F && nodes[i].nF == nodes[0].nF;
    std::vector<double>& Fp = c->stage_f;
    std::vector<double>& rest = c->stage_rest;       // [ls | scale | noise | targets]
    const size_t ls_n = (size_t)std::max(nF_max, 1) * count;
    rest.resize(ls_n + 2 * (size_t)count + n * (size_t)count);
    double* lsp = rest.data();
    double* sc = lsp + ls_n;
    double* no = sc + count;
    double* tg = no + count;
    std::fill(lsp, lsp + ls_n, 1.0);
    if (!same_f) {
        Fp.resize(n * (size_t)nF_max * count);
        std::fill(Fp.begin(), Fp.end(), 0.0);
    }
    for (int i = 0; i < count; ++i) {
        const gpslc_node& q = nodes[i];
        if (q.nF > 0) {
            if (!same_f) memcpy(Fp.data() + (size_t)i * n * nF_max, q.F, n * (size_t)q.nF * sizeof(double));
            memcpy(lsp + (size_t)i * nF_max, q.ls, (size_t)q.nF * sizeof(double));
        }
        sc[i] = q.scale; no[i] = q.noise;
        memcpy(tg + (size_t)i * n, q.target, n * sizeof(double));
    }
    const double* Fsrc = nF_max == 0 ? nullptr : (same_f ? nodes[0].F : Fp.data());
    if (!grad_or_null)
        return gp_logpdf_general(c, count, nF_max, Fsrc, same_f ? 1 : 0, nF_max ? lsp : nullptr, sc, no, tg, 0, logpdf, draws_or_null);
    // The gradient comes back in the padded layout (count sets of nF_max columns, one block per node even where the nodes share
    // their features); the padding columns' gradients are dropped here.  A real column's sums do not see the padding: K adds
    // +0.0 per padding column and every feature is summed on its own, so a node's bits do not depend on the widest node.
    const NodeGradOut& g = *grad_or_null;
    std::vector<double> pF(g.dF ? n * (size_t)nF_max * count : 0), pls(g.dls ? (size_t)nF_max * count : 0);
    const NodeGradOut padded{g.dF ? pF.data() : nullptr, g.dls ? pls.data() : nullptr, g.dscale, g.dnoise, g.dtarget};
    const int st = gp_logpdf_general(c, count, nF_max, Fsrc, same_f ? 1 : 0, nF_max ? lsp : nullptr, sc, no, tg, 0, logpdf, nullptr, &padded);
    size_t fo = 0, lo = 0;
    for (int i = 0; i < count && st >= 0; ++i) {
        const size_t nF = (size_t)nodes[i].nF;
        if (g.dF && nF) memcpy(g.dF + fo, pF.data() + (size_t)i * n * nF_max, n * nF * sizeof(double));
        if (g.dls && nF) memcpy(g.dls + lo, pls.data() + (size_t)i * nF_max, nF * sizeof(double));
        fo += n * nF; lo += nF;
    }
    return st;
}

// The argument checks of the fused node calls (`out`: the output the call must deliver, argument 4 of both signatures):
// the largest feature count of the nodes, or the negative status
int nodes_check(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, const double* out, const char* out_is_null) {
    if (!c) return -1;
    if (count < 0) return bad_arg(c, 2, "count < 0");
    if (count > 0 && !nodes) return bad_arg(c, 3, "nodes is NULL");
    if (count > 0 && !out) return bad_arg(c, 4, out_is_null);
    int nF_max = 0;
    for (int i = 0; i < count; ++i) {
        const gpslc_node& q = nodes[i];
        if (q.nF < 0 || q.nF > 32 || (q.nF > 0 && (!q.F || !q.ls)) || !q.target)
            return bad_arg(c, 3, "node with nF outside 0..32 or a NULL feature / lengthscale / target pointer");
        nF_max = std::max(nF_max, (int)q.nF);
    }
    return nF_max;
}

// The body of the fused node calls: every node one workgroup of ONE launch, or — beyond the single-workgroup kernels (n > 640,
// many nodes, fp32 kernel mode) — the batched tiled factorisation of every node's covariance; with draws_or_null also
// chol(K_i) target_i per node (the small kernels' draw mode; L z on the predictive-draw kernel, round 6)
int nodes_score(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, int nF_max, double* logpdf_or_null, double* draws_or_null) {
    if (count == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        std::vector<double> lp;                      // the scores are computed either way: kept only when the caller asks
        if (!logpdf_or_null) { lp.resize((size_t)count); logpdf_or_null = lp.data(); }
        if (!fast_path_ok(c, nF_max, count)) return nodes_general(c, count, nodes, nF_max, logpdf_or_null, draws_or_null);
        std::vector<HostNode> hn;
        hn.reserve((size_t)count);
        for (int i = 0; i < count; ++i) {
            const gpslc_node& q = nodes[i];
            hn.push_back(rbf_node(q.nF, q.F, q.ls, q.scale, q.noise, q.target));
        }
        return small_nodes_logpdf(c, count, hn.data(), logpdf_or_null, draws_or_null);
    });
}

// both paths of gpslc_mvn_logpdf / gpslc_mvn_draw can run on this ctx (n <= 640): then the dense covariance is always kept
bool mvn_dual(const gpslc_ctx* c) { return fast_path_ok(c, 0, 1); }

// the tiled factor of the device covariance dcov (substitution-based: SigmaU * uNoise is near-singular by construction, 1e-13
// jitter, src/utils.jl:17-33); mvn.logdet / mvn.info from it, and it now stands for hand-over mvn.gen
void mvn_factor_tiles(gpslc_ctx* c, const double* dcov) {
    ensure_streams(c);
    const int nt = c->nt;
    const long long nlow = (long long)nt * (nt + 1) / 2;
    StreamSlot& slot = c->slots[0];
    hipStream_t st = slot.st;
    c->mvn.tiles_gen = 0;
    c->mvn.tiles.reserve((size_t)nlow * GP_TSQ * 8);
    DevBuffer<double> old, oq;
    DevBuffer<int> info;
    old.reserve(8); oq.reserve(8); info.reserve(sizeof(int));
    HC(hipMemsetAsync(info, 0, sizeof(int), st));
    TRef M = lower_ref(c->mvn.tiles, nlow * GP_TSQ);
    launch_dense_load(DenseLoadArgs{dcov, (int)c->n, nt, M}, st);
    factor_robust(c, slot, M, nt, info, 0, 1, 0);
    launch_quad_rows(QuadRowsArgs{M, (int)c->n, nt, 0, 0, old, oq}, st);
    HC(hipStreamSynchronize(st));
    HC(hipGetLastError());
    HC(hipMemcpy(&c->mvn.logdet, old, 8, hipMemcpyDeviceToHost));
    HC(hipMemcpy(&c->mvn.info, info, sizeof(int), hipMemcpyDeviceToHost));
    c->mvn.tiles_gen = c->mvn.gen;
}

// the tiled solve of gpslc_mvn_logpdf against the cached factor: z_s = L^-1 x_s for all S vectors (host, n x S) as the rows of
// W = X^T L^-T, a tile-level solve; returns |z_s|^2 (device, S values in the ctx's staging pool), the stream drained
const double* mvn_solve_tiles(gpslc_ctx* c, int64_t S, const double* x) {
    ensure_streams(c);
    const int n = (int)c->n, nt = c->nt;
    const long long nlow = (long long)nt * (nt + 1) / 2;
    StreamSlot& slot = c->slots[0];
    hipStream_t st = slot.st;
    const int naug = (int)((S + GP_TS - 1) / GP_TS);
    c->io.reset();
    const double* dx = up(c, x, (size_t)n * S);
    double* wt = c->io.take<double>((size_t)naug * nt * GP_TSQ);
    double* oq = c->io.take<double>((size_t)S);
    TRef W = rect_ref(wt, (long long)naug * nt * GP_TSQ, nt);
    TRef Ls = lower_ref(c->mvn.tiles, nlow * GP_TSQ);
    launch_rows_rhs(RowsRhsArgs{dx, S, n, nt, naug, W, 0, 1}, st);
    const int short_rows = naug == 1 ? (int)S : 0;
    // right-looking: z_k = w_k L_kk^-T by substitution (no inverted block: the factor is near-singular), then every
    // remaining column block in parallel on the MFMA tile kernel
    for (int k = 0; k < nt; ++k) {
        launch_trsm_robust(W, Ls, k, 0, naug, 1, st);
        if (k + 1 < nt)     // W(:, j) -= W(:, k) L(j, k)^T for j > k
            gemm(c, short_aug_row(tile_rect(W, Ls, W, 0, k + 1, naug, nt - k - 1, k, k + 1, 1), 0, short_rows), slot, 0);
    }
    launch_row_norms(RowNormArgs{W, nt, naug, S, oq}, st);
    HC(hipStreamSynchronize(st));
    HC(hipGetLastError());
    return oq;
}

// hands a covariance over: n <= 640 keeps the dense matrix (and validates it on the single-workgroup kernel when the call takes
// that path), the tiled path factorises it; mvn.info = its LAPACK-style info
void mvn_cache(gpslc_ctx* c, const double* cov, bool small) {
    const size_t n = (size_t)c->n;
    c->mvn.valid = false;
    ++c->mvn.gen;
    if (!mvn_dual(c)) {      // n > 640 (or the fp32 kernel mode): the tiled path is the only one
        DevBuffer<double> bcov;
        mvn_factor_tiles(c, up(bcov, cov, n * n));
        c->mvn.valid = true;
        return;
    }
    c->mvn.dense.reserve(n * n * sizeof(double));
    HC(hipMemcpy(c->mvn.dense, cov, n * n * sizeof(double), hipMemcpyHostToDevice));
    if (small) {
        // validate once (as the tiled path does when it factorises): info of cov itself
        std::vector<double> zeros(n, 0.0);
        const HostNode probe = dense_node(c->mvn.dense, 1.0, zeros.data());
        double dummy = 0.0;
        c->mvn.info = small_nodes_logpdf(c, 1, &probe, &dummy);
    } else {
        mvn_factor_tiles(c, c->mvn.dense);
    }
    c->mvn.valid = true;
}

// before a cov = NULL call on the tiled path: the factor of the latest hand-over (rebuilt from the dense copy when an earlier
// hand-over went to the single-workgroup path)
void mvn_tiles_current(gpslc_ctx* c) {
    if (c->mvn.tiles && c->mvn.tiles_gen == c->mvn.gen) return;
    mvn_factor_tiles(c, c->mvn.dense);
}

// What gpslc_mvn_logpdf and gpslc_mvn_draw do before they differ (`in`: x / z, argument 5; `out`: the result, argument 6):
// the pointer checks, then — small: the call runs on the single-workgroup kernels — the covariance is handed over, or the tiled
// factor brought up to date when the call runs tiled and gave none, and every vector's info is that of the covariance.
// `body(small)` goes on from there; mvn.info != 0 and S == 0 are its to answer (the two calls differ there).
template <class Body>
int mvn_call(gpslc_ctx* c, int64_t S, const double* cov, const double* in, const char* in_is_null, const double* out,
             const char* out_is_null, Body&& body) {
    if (!c) return -1;
    if (S < 0) return bad_arg(c, 2, "S < 0");
    if (!cov && !c->mvn.valid) return bad_arg(c, 3, "cov is NULL and no factor is cached");
    if (S > 0 && !in) return bad_arg(c, 5, in_is_null);
    if (S > 0 && !out) return bad_arg(c, 6, out_is_null);
    const bool small = fast_path_ok(c, 0, std::max<int64_t>(S, 1));
    return guarded(c, [&]() {
        if (cov) mvn_cache(c, cov, small);   // factor once, keep it in the context
        else if (!small) mvn_tiles_current(c);
        c->last_info.assign((size_t)S, c->mvn.info);
        return body(small);
    });
}

// the S dense-covariance nodes of the single-workgroup path: covscale_s times the cached covariance, target column s
std::vector<HostNode> mvn_nodes(const gpslc_ctx* c, int64_t S, const double* covscale, const double* target) {
    std::vector<HostNode> hn;
    hn.reserve((size_t)S);
    for (int64_t s = 0; s < S; ++s) hn.push_back(dense_node(c->mvn.dense, covscale ? covscale[s] : 1.0, target + s * c->n));
    return hn;
}

}  // namespace

extern "C" {

int gpslc_y_logpdf(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                   const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale,
                   const double* yNoise, double* logpdf) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!logpdf) return bad_arg(c, 11, "logpdf is NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    if (!fast_path_ok(c, c->nU + c->nX + 1, S)) {
        PredictIO io;
        return outcome_call(c, rq, X_or_null, Y_or_null, logpdf, io, {});
    }
    return guarded(c, [&]() {
        // small n: every parameter set is one workgroup of ONE launch (k_small.hip); T enters as a feature column
        const size_t n = (size_t)c->n;
        std::vector<HostNode> hn;
        hn.reserve((size_t)S);
        for (int64_t s = 0; s < S; ++s)
            hn.push_back(y_node(c->nU, U + s * n * c->nU, uyLS + s * c->nU, c->nX, X_or_null ? X_or_null : c->hX.data(),
                                xyLS + s * c->nX, c->hT.data(), tyLS[s], yScale[s], yNoise[s],
                                Y_or_null ? Y_or_null : c->hY.data()));
        return small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
    });
}

// leave-one-out checks from the tile factor gpslc_y_logpdf's general path computes: the tiled path at every n
int gpslc_y_loo(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                double* looMean, double* looVar, double* looLpd, double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!looMean && !looVar && !looLpd && !logpdf_or_null) return bad_arg(c, 11, "looMean, looVar, looLpd and logpdf are all NULL");
    const size_t nS = (size_t)c->n * (size_t)S;
    PredictIO io;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{looMean, &io.loo.mean, nS}, {looVar, &io.loo.var, nS}, {looLpd, &io.loo.lpd, nS}});
}

// gradient of the outcome log-likelihood: gpslc_y_loo's call with other outputs
int gpslc_y_logpdf_grad(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                        const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                        double* dU, double* duyLS, double* dxyLS, double* dtyLS, double* dyScale, double* dyNoise, double* dY,
                        double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    if (!dU && !duyLS && !dxyLS && !dtyLS && !dyScale && !dyNoise && !dY)
        return bad_arg(c, 11, "dU, duyLS, dxyLS, dtyLS, dyScale, dyNoise and dY are all NULL");
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) {
        set_err(c, "gpslc_y_logpdf_grad needs an fp64 context: the pair pass evaluates K in fp64, not the matrix an fp32 context factorises");
        return GPSLC_ERR_UNSUPPORTED;
    }
    if (c->nU == 0) dU = duyLS = nullptr;       // the outputs of an empty block are ignored
    if (c->nX == 0) dxyLS = nullptr;
    const size_t sS = (size_t)S, nS = (size_t)c->n * sS;
    PredictIO io;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{dU, &io.grad.U, nS * (size_t)c->nU}, {duyLS, &io.grad.uyLS, (size_t)c->nU * sS},
                         {dxyLS, &io.grad.xyLS, (size_t)c->nX * sS}, {dtyLS, &io.grad.tyLS, sS}, {dyScale, &io.grad.yScale, sS},
                         {dyNoise, &io.grad.yNoise, sS}, {dY, &io.grad.Y, nS}});
}

// leave-group-out checks: gpslc_y_loo's call with a labelling; every check before any device work
int gpslc_y_lgo(gpslc_ctx* c, int64_t S, const double* U, const double* X_or_null, const double* Y_or_null,
                const double* uyLS, const double* xyLS, const double* tyLS, const double* yScale, const double* yNoise,
                int32_t G, const int32_t* labels, double* lgoMean, double* lgoVar, double* lgoLpd, double* logpdf_or_null) {
    const PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, 0, nullptr);
    int rc = validate(c, rq, kSamplesArgs);
    if (rc) return rc;
    const int64_t n = c->n;
    if (G < 1 || G > n) return bad_arg(c, 11, "G < 1 or G > n");
    if (!labels) return bad_arg(c, 12, "labels is NULL");
    // the member list sorted by (group, row): a counting sort, rows ascending inside every group
    std::vector<int> offsets((size_t)G + 1, 0), members((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] < 0 || labels[i] >= G) return bad_arg(c, 12, "a label is outside [0, G)");
        ++offsets[(size_t)labels[i] + 1];
    }
    for (int32_t g = 0; g < G; ++g) {
        if (offsets[(size_t)g + 1] == 0) return bad_arg(c, 12, "a group has no member");
        offsets[(size_t)g + 1] += offsets[g];
    }
    if (!lgoMean && !lgoVar && !lgoLpd) return bad_arg(c, 13, "lgoMean, lgoVar and lgoLpd are all NULL");
    PredictIO io;
    io.lgo.G = G;
    for (int32_t g = 0; g < G; ++g) {
        const int m = offsets[(size_t)g + 1] - offsets[g];
        io.lgo.mmax = std::max(io.lgo.mmax, m);
        if (m > LGO_MAX_GROUP) {
            char buf[160];
            snprintf(buf, sizeof buf, "group %d has %d members: gpslc_y_lgo takes groups of at most %d", (int)g, m, LGO_MAX_GROUP);
            set_err(c, buf);
            return GPSLC_ERR_UNSUPPORTED;
        }
    }
    {
        std::vector<int> fill(offsets.begin(), offsets.end() - 1);
        for (int64_t i = 0; i < n; ++i) members[(size_t)fill[labels[i]]++] = (int)i;
    }
    const size_t nS = (size_t)n * (size_t)S, GS = (size_t)G * (size_t)S;
    return outcome_call(c, rq, X_or_null, Y_or_null, logpdf_or_null, io,
                        {{lgoMean, &io.lgo.mean, nS}, {lgoVar, &io.lgo.var, nS}, {lgoLpd, &io.lgo.lpd, GS}}, [&]() {
                            auto upload = [&](const std::vector<int>& v) {      // the member list and its offsets
                                int* d = c->io.take<int>(v.size());
                                HC(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
                                return d;
                            };
                            io.lgo.members = upload(members); io.lgo.offsets = upload(offsets);
                        });
}

// The checks gpslc_predict_new and gpslc_predict_new_weighted share: the samples, then arguments 9 - 15 (m, Xnew, Unew, form, L,
// doT, doT_base), which sit at the same positions in both
static int validate_new(gpslc_ctx* c, const PredictRequest& rq, int64_t m, const double* Xnew, const double* Unew, int32_t form,
                        const double* doT_base) {
    static const ArgPos kNewArgs{2, 3, 5, 6, 13, 14, 0, 0, 0, 0, true};
    const int64_t S = rq.post.S;
    const int32_t L = rq.lv.L;
    const double* doT = rq.lv.doT;
    int rc = validate(c, rq, kNewArgs);
    if (rc) return rc;
    if (m < 1 || m > (int64_t)GP_TS * 32767) return bad_arg(c, 9, "m < 1 (or beyond 32767 row tiles)");
    if ((c->nX > 0) != (Xnew != nullptr)) return bad_arg(c, 10, c->nX > 0 ? "Xnew is NULL but nX > 0" : "Xnew given but nX == 0");
    if (Xnew && (rc = finite_check(c, Xnew, m * c->nX, 10, "Xnew"))) return rc;
    if ((c->nU > 0) != (Unew != nullptr)) return bad_arg(c, 11, c->nU > 0 ? "Unew is NULL but nU > 0" : "Unew given but nU == 0");
    if (Unew && (rc = finite_check(c, Unew, m * c->nU * S, 11, "Unew"))) return rc;
    if (form != GPSLC_NEW_OUTCOME && form != GPSLC_NEW_CONTRAST && form != GPSLC_NEW_SLOPE)
        return bad_arg(c, 12, "unknown form (GPSLC_NEW_OUTCOME, GPSLC_NEW_CONTRAST or GPSLC_NEW_SLOPE: the ordinary effect f(a) - f(T) "
                              "needs a factual treatment, which a new individual does not have)");
    if ((rc = finite_check(c, doT, L, 14, "doT"))) return rc;
    if (form == GPSLC_NEW_CONTRAST) {
        if ((rc = finite_check(c, doT_base, L, 15, "doT_base"))) return rc;
    } else if (doT_base) {
        return bad_arg(c, 15, "doT_base given for a form that is no contrast");
    }
    return 0;
}
// ... and their uploads: the samples, the levels of the form and the new individuals' features
static PredictIO new_io(gpslc_ctx* c, const PredictRequest& rq, int64_t m, const double* Xnew, const double* Unew, int32_t form,
                        const double* doT_base, double pred_noise) {
    const size_t mm = (size_t)m, S = (size_t)rq.post.S, L = (size_t)rq.lv.L;
    PredictIO io;
    io.post.S = rq.post.S; io.post.p = upload_samples(c, rq.post.p, 0, S);
    io.X = c->dX;
    io.lv.L = rq.lv.L; io.lv.doT = up(c, rq.lv.doT, L);
    io.lv.form = form == GPSLC_NEW_OUTCOME ? FORM_OUTCOME : form == GPSLC_NEW_SLOPE ? FORM_SLOPE : FORM_CONTRAST;
    io.lv.base = doT_base ? up(c, doT_base, L) : nullptr;
    io.out.pred_noise = pred_noise;
    io.fresh.m = (int)m;
    io.fresh.Xnew = Xnew ? up(c, Xnew, mm * c->nX) : nullptr;
    io.fresh.Unew = Unew ? up(c, Unew, mm * c->nU * S) : nullptr;
    return io;
}

// predictions for m new individuals: host pointers; every check before any device work
int gpslc_predict_new(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                      const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                      int32_t form, int32_t L, const double* doT, const double* doT_base, double pred_noise, double* mean,
                      double* var, double* cov) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    int rc = validate_new(c, rq, m, Xnew, Unew, form, doT_base);
    if (rc) return rc;
    if (!std::isfinite(pred_noise)) return bad_arg(c, 16, "pred_noise is not finite");
    if (!mean && !var && !cov) return bad_arg(c, 17, "mean, var and cov are all NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t mm = (size_t)m, SL = (size_t)S * L;
        c->io.reset();
        PredictIO io = new_io(c, rq, m, Xnew, Unew, form, doT_base, pred_noise);
        const Outputs outs = {{mean, &io.fresh.mean, mm * SL}, {var, &io.fresh.var, mm * SL}, {cov, &io.fresh.cov, mm * mm * SL}};
        take_outputs(c, outs);
        if (cov && !var) io.fresh.var = c->io.take<double>(mm * SL);      // the covariance takes its diagonal from it
        io.info = c->io.take<int>((size_t)S);
        run_predict(c, io);
        const int st = first_info(c);
        deliver_outputs(c, outs);
        if (st > 0)      // a sample whose factorisation broke down: NaN in everything of it
            for (int64_t s = 0; s < S; ++s) {
                if (c->last_info[(size_t)s] == 0) continue;
                for (int64_t l = 0; l < L; ++l) {
                    const size_t o = mm * (size_t)(s + S * l);
                    if (mean) std::fill(mean + o, mean + o + mm, NAN);
                    if (var) std::fill(var + o, var + o + mm, NAN);
                    if (cov) std::fill(cov + mm * o, cov + mm * (o + mm), NAN);
                }
            }
        return st;
    });
}

// weighted averages over m new individuals: gpslc_predict_new's checks, then G >= 1 columns of m finite weights
int gpslc_predict_new_weighted(gpslc_ctx* c, int64_t S, const double* U, const double* uyLS, const double* xyLS, const double* tyLS,
                               const double* yScale, const double* yNoise, int64_t m, const double* Xnew, const double* Unew,
                               int32_t form, int32_t L, const double* doT, const double* doT_base, int32_t G, const double* weights,
                               double pred_noise, double* meanW, double* varW, double* covW) {
    PredictRequest rq = make_request(S, {U, uyLS, xyLS, tyLS, yScale, yNoise}, L, doT);
    int rc = validate_new(c, rq, m, Xnew, Unew, form, doT_base);
    if (rc) return rc;
    if (G < 1) return bad_arg(c, 16, "G < 1");
    if ((rc = finite_check(c, weights, m * (int64_t)G, 17, "weights"))) return rc;
    if (!std::isfinite(pred_noise)) return bad_arg(c, 18, "pred_noise is not finite");
    if (!meanW && !varW && !covW) return bad_arg(c, 19, "meanW, varW and covW are all NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t mm = (size_t)m, Gs = (size_t)G, SR = (size_t)S * L * Gs;
        c->io.reset();
        PredictIO io = new_io(c, rq, m, Xnew, Unew, form, doT_base, pred_noise);
        io.fresh.weighted = true;
        {       // m x G host (weights[i + m*g]) -> column fastest on the device (W[g + G*i]), as predict_host does
            std::vector<double> wt(mm * Gs);
            for (size_t i = 0; i < mm; ++i)
                for (size_t g = 0; g < Gs; ++g) wt[g + Gs * i] = weights[i + mm * g];
            io.lv.W = up(c, wt.data(), wt.size());
            io.lv.G = G;
        }
        const Outputs outs = {{meanW, &io.out.meanSATE, SR}, {varW, &io.out.varSATE, SR}, {covW, &io.out.covW, SR * L}};
        take_outputs(c, outs);
        if (covW && !varW) io.out.varSATE = c->io.take<double>(SR);      // the joint covariance takes its diagonal from it
        io.info = c->io.take<int>((size_t)S);
        run_predict(c, io);
        const int st = first_info(c);
        deliver_outputs(c, outs);
        if (st > 0)      // a sample whose factorisation broke down: NaN in everything of it (sample fastest in every output)
            for (const Output& o : outs)
                for (size_t s = 0; o.host && s < (size_t)S; ++s)
                    if (c->last_info[s] != 0)
                        for (size_t k = s; k < o.count; k += (size_t)S) o.host[k] = NAN;
        return st;
    });
}

int gpslc_gp_logpdf(gpslc_ctx* c, int64_t S, int32_t nF, const double* F, int32_t f_shared, const double* ls,
                    const double* scale, const double* noise, const double* target, int32_t t_shared,
                    double* logpdf) {
    if (!c) return -1;
    if (S < 0) return bad_arg(c, 2, "S < 0");
    if (nF < 0 || nF > 32) return bad_arg(c, 3, "nF must be in 0..32");
    if (nF > 0 && (!F || !ls)) return bad_arg(c, 4, "F / ls must not be NULL when nF > 0");
    if (S > 0 && (!scale || !noise)) return bad_arg(c, 7, "scale / noise must not be NULL");
    if (S > 0 && !target) return bad_arg(c, 9, "target is NULL");
    if (!logpdf) return bad_arg(c, 11, "logpdf is NULL");
    if (S == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        const size_t n = (size_t)c->n;
        if (!fast_path_ok(c, nF, S)) return gp_logpdf_general(c, S, nF, F, f_shared, ls, scale, noise, target, t_shared, logpdf);
        std::vector<HostNode> hn;
        hn.reserve((size_t)S);
        for (int64_t s = 0; s < S; ++s)
            hn.push_back(rbf_node(nF, F + (f_shared ? 0 : s * n * nF), ls + s * nF, scale[s], noise[s], target + (t_shared ? 0 : s * n)));
        return small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
    });
}

int gpslc_nodes_logpdf(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* logpdf) {
    const int nF_max = nodes_check(c, count, nodes, logpdf, "logpdf is NULL");
    return nF_max < 0 ? nF_max : nodes_score(c, count, nodes, nF_max, logpdf, nullptr);
}

// The fused whole-model gradient: the score's single launch with the gradient phases behind it while every node
// fits small_grad_lds_bytes, else — one node that does not fit, more than 4096 nodes — the tiled path for the whole call
int gpslc_nodes_logpdf_grad(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* dF, double* dls, double* dscale,
                            double* dnoise, double* dtarget, double* logpdf_or_null) {
    const NodeGradOut g{dF, dls, dscale, dnoise, dtarget};
    const double* some = g.any() ? (dF ? dF : dls ? dls : dscale ? dscale : dnoise ? dnoise : dtarget) : nullptr;
    const int nF_max = nodes_check(c, count, nodes, some, "dF, dls, dscale, dnoise and dtarget are all NULL");
    if (nF_max < 0) return nF_max;
    if (c->flags & GPSLC_FLAG_FP32_KERNEL) {
        set_err(c, "gpslc_nodes_logpdf_grad needs an fp64 context: the gradient evaluates K in fp64, not the matrix an fp32 context factorises");
        return GPSLC_ERR_UNSUPPORTED;
    }
    if (count == 0) { c->last_info.clear(); return GPSLC_OK; }
    return guarded(c, [&]() {
        std::vector<double> lp;
        double* logpdf = logpdf_or_null;
        if (!logpdf) { lp.resize((size_t)count); logpdf = lp.data(); }
        if (small_grad_lds_bytes((int)c->n, nF_max) > kLdsCapBytes || count > 4096)
            return nodes_general(c, count, nodes, nF_max, logpdf, nullptr, &g);
        std::vector<HostNode> hn;
        hn.reserve((size_t)count);
        for (int i = 0; i < count; ++i) {
            const gpslc_node& q = nodes[i];
            hn.push_back(rbf_node(q.nF, q.F, q.ls, q.scale, q.noise, q.target));
        }
        return small_nodes_logpdf(c, count, hn.data(), logpdf, nullptr, &g);
    });
}

int gpslc_nodes_draw(gpslc_ctx* c, int32_t count, const gpslc_node* nodes, double* draws, double* logpdf_or_null) {
    const int nF_max = nodes_check(c, count, nodes, draws, "draws is NULL");
    return nF_max < 0 ? nF_max : nodes_score(c, count, nodes, nF_max, logpdf_or_null, draws);
}

int gpslc_mvn_logpdf(gpslc_ctx* c, int64_t S, const double* cov, const double* covscale, const double* x,
                     double* logpdf) {
    return mvn_call(c, S, cov, x, "x is NULL", logpdf, "logpdf is NULL", [&](bool small) {
        if (S == 0 || c->mvn.info != 0) {
            for (int64_t s = 0; s < S; ++s) logpdf[s] = NAN;
            return c->mvn.info;
        }
        if (small) {
            // small n: the dense matrix stays on the device; every evaluation is one workgroup that scales, factorises
            // and solves in LDS (k_small.hip) — cheaper than the tiled forward solve against a cached factor
            const std::vector<HostNode> hn = mvn_nodes(c, S, covscale, x);
            const int st = small_nodes_logpdf(c, (int)S, hn.data(), logpdf);
            if (st > 0) for (int64_t s = 0; s < S; ++s) if (c->last_info[s] != 0) logpdf[s] = NAN;
            return st;
        }
        const int n = (int)c->n;
        const double* oq = mvn_solve_tiles(c, S, x);
        if (c->flags & GPSLC_FLAG_PROFILE) prof_collect(c);
        std::vector<double> q(S);
        HC(hipMemcpy(q.data(), oq, sizeof(double) * S, hipMemcpyDeviceToHost));
        for (int64_t s = 0; s < S; ++s) {
            const double sc = covscale ? covscale[s] : 1.0;
            logpdf[s] = -0.5 * ((double)n * kLog2Pi + (double)n * std::log(sc) + c->mvn.logdet + q[s] / sc);
        }
        return GPSLC_OK;
    });
}

// draws[:, s] = chol(covscale_s cov) z[:, s]: Gen's mvnormal(zeros(n), uCov) with the host's normals — the auxiliary vector of
// elliptical_slice(trace, :U => k => :U, zeros(n), uCov) (src/inference.jl:48-54) and the prior draw generateUfromSigmaU
// (src/model_likelihood.jl:4-10) — from the covariance gpslc_mvn_logpdf caches (chol(s C) = sqrt(s) chol(C))
int gpslc_mvn_draw(gpslc_ctx* c, int64_t S, const double* cov, const double* covscale, const double* z, double* draws) {
    return mvn_call(c, S, cov, z, "z is NULL", draws, "draws is NULL", [&](bool small) {
        const size_t n = (size_t)c->n;
        if (S == 0) return GPSLC_OK;        // a hand-over alone answers GPSLC_OK here; the covariance's info is in last_info
        if (c->mvn.info != 0) {
            for (size_t e = 0; e < n * (size_t)S; ++e) draws[e] = NAN;
            return c->mvn.info;
        }
        if (small) {
            const std::vector<HostNode> hn = mvn_nodes(c, S, covscale, z);
            std::vector<double> lp((size_t)S);
            return small_nodes_logpdf(c, (int)S, hn.data(), lp.data(), draws);
        }
        // tiled: L z on the predictive-draw kernel (every unit streams the ONE cached factor: batch stride 0), scaled on the host
        ensure_streams(c);
        hipStream_t st = c->slots[0].st;
        const int nt = c->nt;
        const long long Np = (long long)nt * GP_TS;
        c->io.reset();
        const double* dz = up(c, z, n * (size_t)S);
        double* zero_mean = c->io.take<double>(n * (size_t)S);
        double* out = c->io.take<double>(n * (size_t)S);
        double* zt = c->io.take<double>((size_t)S * draws_image_doubles(1, Np));
        HC(hipMemsetAsync(zero_mean, 0, n * (size_t)S * sizeof(double), st));
        launch_draws(zero_mean_draw(lower_ref(c->mvn.tiles, 0), (int)n, nt, 0, S, zero_mean, dz, zt, out), (int)S, st);
        HC(hipStreamSynchronize(st));
        HC(hipGetLastError());
        HC(hipMemcpy(draws, out, n * (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
        if (covscale)
            for (int64_t s = 0; s < S; ++s) {
                const double r = std::sqrt(covscale[s]);
                for (size_t i = 0; i < n; ++i) draws[s * n + i] *= r;
            }
        return GPSLC_OK;
    });
}

// doTv: null = the scalar doT, else the per-individual intervention (n, host)
static int likelihood_distribution_impl(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                        double tyLS, double yScale, double yNoise, double doT, const double* doTv,
                                        double* CovWW, double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                        double* CovC21, double* CovC22) {
    const double ty = tyLS, ysc = yScale, yno = yNoise;
    return guarded(c, [&]() {
        ensure_streams(c);
        StreamSlot& slot = c->slots[0];
        hipStream_t st = slot.st;
        const int n = (int)c->n, nt = c->nt;
        const long long nlow = (long long)nt * (nt + 1) / 2, nsq = (long long)nt * nt;
        DevBuffer<double> bdo, tiles, inv, rect, outb;
        DevBuffer<int> info;
        c->io.reset();
        SampleParams sp = upload_samples(c, SampleParams{U, uyLS, xyLS, &ty, &ysc, &yno}, 0, 1);
        sp.u_sstride = (long long)n * c->nU;
        info.reserve(sizeof(int));
        HC(hipMemsetAsync(info, 0, sizeof(int), st));
        tiles.reserve((size_t)nlow * GP_TSQ * 8);
        inv.reserve((size_t)nt * GP_TSQ * 8);
        rect.reserve((size_t)6 * nsq * GP_TSQ * 8);      // K, Ks, Ks', Kss, W1, W2
        outb.reserve((size_t)n * n * 8);
        double* rb = rect;
        const long long rs = nsq * GP_TSQ;
        TRef Kt = rect_ref(rb, rs, nt), Kst = rect_ref(rb + rs, rs, nt), KsTt = rect_ref(rb + 2 * rs, rs, nt),
             Ksst = rect_ref(rb + 3 * rs, rs, nt), W1 = rect_ref(rb + 4 * rs, rs, nt), W2 = rect_ref(rb + 5 * rs, rs, nt);
        TRef M = lower_ref(tiles, nlow * GP_TSQ);
        // A = K + yNoise I (lower tiles) and its factor
        const SampleGrid grid{c->dX, c->dT, sp, 0, n, c->nX, c->nU, nt};
        GramArgs ga{grid};
        ga.M = M; ga.part = nullptr; ga.with_sums = 0; ga.f32 = 0;
        launch_gram(ga, 1, st);
        factor_panels(c, slot, M, nt, nt, inv, info, 0, 1, 0, false, 0);
        LdBuildArgs la{grid, doT, Kt, Kst, KsTt, Ksst};
        if (doTv) la.doTv = up(bdo, doTv, (size_t)n);
        launch_ld_build(la, st);
        auto emit = [&](const TRef& R, double* host, double diag_add) {
            if (!host) return;
            launch_rect_gather(RectGatherArgs{R, n, nt, outb, diag_add}, st);
            HC(hipStreamSynchronize(st));
            copy_out_large(c, host, outb, (size_t)n * n * 8);
        };
        emit(Kt, CovWW, 0.0);
        emit(Kst, CovWWs, 0.0);
        emit(Kt, CovWWp, yno);
        if (CovC11 || CovC12 || CovC21 || CovC22) {
            // W1 = K L^-T, W2 = Ks' L^-T  (copies, then unit B's tile-level left-looking solve)
            HC(hipMemcpyAsync(W1.base, Kt.base, (size_t)rs * 8, hipMemcpyDeviceToDevice, st));
            HC(hipMemcpyAsync(W2.base, KsTt.base, (size_t)rs * 8, hipMemcpyDeviceToDevice, st));
            TRef invref = inv_ref(inv, nt);
            w_solve(c, slot, W1, M, invref, nt, 1, nt);
            w_solve(c, slot, W2, M, invref, nt, 1, nt);
            // C11 = K - W1 W1', C12 = Ks - W1 W2', C21 = Ks' - W2 W1', C22 = Kss - W2 W2'   (src/likelihood.jl:46-49)
            auto block = [&](const TRef& Cm, const TRef& Wa, const TRef& Wb, double* host) {
                if (!host) return;
                gemm(c, tile_rect(Wa, Wb, Cm, 0, 0, nt, nt, 0, nt, 1), slot, 0);
                emit(Cm, host, 0.0);
            };
            block(Kt, W1, W1, CovC11);      // K, Ks, Ks', Kss are consumed in place: emitted above already
            block(Kst, W1, W2, CovC12);
            block(KsTt, W2, W1, CovC21);
            block(Ksst, W2, W2, CovC22);
        }
        HC(hipStreamSynchronize(st));
        HC(hipGetLastError());
        int hinfo = 0;
        HC(hipMemcpy(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost));
        c->last_info.assign(1, hinfo);
        return hinfo;
    });
}

int gpslc_likelihood_distribution(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                  double tyLS, double yScale, double yNoise, double doT, double* CovWW,
                                  double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                  double* CovC21, double* CovC22) {
    int rc = validate(c, make_request(1, {U, uyLS, xyLS, &tyLS, &yScale, &yNoise}, 0, nullptr), kSamplesArgs);
    if (rc) return rc;
    return likelihood_distribution_impl(c, U, uyLS, xyLS, tyLS, yScale, yNoise, doT, nullptr, CovWW, CovWWs, CovWWp, CovC11,
                                        CovC12, CovC21, CovC22);
}

int gpslc_likelihood_distribution_vec(gpslc_ctx* c, const double* U, const double* uyLS, const double* xyLS,
                                      double tyLS, double yScale, double yNoise, const double* doT, double* CovWW,
                                      double* CovWWs, double* CovWWp, double* CovC11, double* CovC12,
                                      double* CovC21, double* CovC22) {
    PredictRequest rq = make_request(1, {U, uyLS, xyLS, &tyLS, &yScale, &yNoise}, 1, doT);
    rq.lv.vec = true;
    int rc = validate(c, rq, kLikelihoodVecArgs);
    if (rc) return rc;
    return likelihood_distribution_impl(c, U, uyLS, xyLS, tyLS, yScale, yNoise, 0.0, doT, CovWW, CovWWs, CovWWp, CovC11,
                                        CovC12, CovC21, CovC22);
}

static int summarize_impl(gpslc_ctx* c, const double* dx, int64_t n, int64_t m, int64_t rs, int64_t cs,
                          double ci, double* dmean, double* dlo, double* dhi) {
    ensure_streams(c);
    int mpad = 1;                                     // LDS image of a row (sorted in place): rows up to 16384 samples
    while (mpad < m && mpad < 16384) mpad <<= 1;      // (longer rows: radix select, no image)
    const double lowerQ = (1.0 - ci) / 2.0;          // src/driver.jl:130-131
    const double upperQ = 1.0 - lowerQ;
    launch_summarize(SummArgs{dx, rs, cs, (int)n, (int)m, mpad, lowerQ, upperQ, dmean, dlo, dhi}, c->slots[0].st);
    HC(hipStreamSynchronize(c->slots[0].st));
    HC(hipGetLastError());
    return GPSLC_OK;
}

int gpslc_summarize_dev(gpslc_ctx* c, const double* samples, int64_t n, int64_t m, int64_t row_stride,
                        int64_t col_stride, double credible_interval, double* mean, double* lower, double* upper) {
    if (!c) return -1;
    if (!samples) return bad_arg(c, 2, "samples is NULL");
    if (n < 1 || n > 2147483647LL) return bad_arg(c, 3, "n must be in 1..2^31-1");
    if (m < 1 || m > 2147483647LL) return bad_arg(c, 4, "m must be in 1..2^31-1");
    if (row_stride < 1) return bad_arg(c, 5, "row_stride < 1");
    if (col_stride < 1) return bad_arg(c, 6, "col_stride < 1");
    if (!(credible_interval > 0.0 && credible_interval < 1.0)) return bad_arg(c, 7, "credible_interval not in (0,1)");
    if (!mean || !lower || !upper) return bad_arg(c, 8, "output is NULL");
    return guarded(c, [&]() { return summarize_impl(c, samples, n, m, row_stride, col_stride, credible_interval,
                                                    mean, lower, upper); });
}

int gpslc_summarize(gpslc_ctx* c, const double* samples, int64_t n, int64_t m, double credible_interval,
                    double* mean, double* lower, double* upper) {
    if (!c) return -1;
    if (!samples) return bad_arg(c, 2, "samples is NULL");
    if (n < 1 || n > 2147483647LL) return bad_arg(c, 3, "n must be in 1..2^31-1");
    if (m < 1 || m > 2147483647LL) return bad_arg(c, 4, "m must be in 1..2^31-1");
    if (!(credible_interval > 0.0 && credible_interval < 1.0)) return bad_arg(c, 5, "credible_interval not in (0,1)");
    if (!mean || !lower || !upper) return bad_arg(c, 6, "output is NULL");
    return guarded(c, [&]() {
        DevBuffer<double> bx, o;
        const double* dx = up(bx, samples, (size_t)n * m);
        o.reserve(sizeof(double) * 3 * n);
        double* d = o;
        summarize_impl(c, dx, n, m, 1, n, credible_interval, d, d + n, d + 2 * n);
        HC(hipMemcpy(mean, d, sizeof(double) * n, hipMemcpyDeviceToHost));
        HC(hipMemcpy(lower, d + n, sizeof(double) * n, hipMemcpyDeviceToHost));
        HC(hipMemcpy(upper, d + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost));
        return GPSLC_OK;
    });
}

int gpslc_sate_samples(const double* meanSATE, const double* varSATE, int64_t S, int32_t spp, uint64_t seed,
                       const double* z, double* out) {
    if (!meanSATE) return -1;
    if (!varSATE) return -2;
    if (S < 0) return -3;
    if (spp < 0) return -4;
    if (!out) return -7;
    for (int64_t j = 0; j < S; ++j)
        for (int32_t d = 0; d < spp; ++d) {
            const int64_t i = j * spp + d;
            const double zz = z ? z[i] : philox_normal(seed, (1ull << 40) + (uint64_t)j, (uint64_t)d);
            out[i] = meanSATE[j] + varSATE[j] * zz;   // variance used as sigma: src/estimation.jl:159
        }
    return GPSLC_OK;
}

// Joint draws of the curve from the (s, g) blocks of gpslc_predict_curve: diagonally pivoted Cholesky of each L x L block,
// stopped at the first pivot <= L eps max diag (the remaining columns of the factor stay zero), mapped back to level order
int gpslc_curve_samples(const double* meanW, const double* covW, int64_t S, int32_t L, int32_t G, int32_t spp, uint64_t seed,
                        const double* z, double* out) {
    if (!meanW) return -1;
    if (!covW) return -2;
    if (S < 0) return -3;
    if (L < 1) return -4;
    if (G < 1) return -5;
    if (spp < 0) return -6;
    if (!out) return -9;
    const size_t Ls = (size_t)L;
    std::vector<double> Cb(Ls * Ls), F(Ls * Ls), dk(Ls);      // dk[i]: the remaining diagonal of level piv[i]
    std::vector<int32_t> piv(Ls);
    for (int32_t g = 0; g < G; ++g)
        for (int64_t s = 0; s < S; ++s) {
            // block (s, g), lower triangle read; Cb and F are indexed in level order, column-major
            double dmax = 0.0;
            for (size_t lp = 0; lp < Ls; ++lp)
                for (size_t l = lp; l < Ls; ++l) {
                    Cb[l + Ls * lp] = covW[(size_t)s + (size_t)S * (l + Ls * (lp + Ls * (size_t)g))];
                    if (l == lp) dmax = std::max(dmax, Cb[l + Ls * lp]);
                }
            std::fill(F.begin(), F.end(), 0.0);
            for (size_t l = 0; l < Ls; ++l) piv[l] = (int32_t)l;
            const double stop = (double)L * 2.220446049250313e-16 * dmax;
            auto c_at = [&](size_t i, size_t j) { return i >= j ? Cb[i + Ls * j] : Cb[j + Ls * i]; };
            for (size_t i = 0; i < Ls; ++i) dk[i] = c_at(i, i);
            size_t rank = 0;
            for (size_t k = 0; k < Ls; ++k) {
                size_t m = k;
                for (size_t i = k + 1; i < Ls; ++i)
                    if (dk[i] > dk[m]) m = i;      // first largest
                if (!(dk[m] > stop)) break;
                std::swap(piv[k], piv[m]);
                std::swap(dk[k], dk[m]);
                const size_t pk = (size_t)piv[k];
                const double lkk = std::sqrt(dk[k]);
                F[pk + Ls * k] = lkk;
                for (size_t i = k + 1; i < Ls; ++i) {
                    const size_t pi = (size_t)piv[i];
                    double v = c_at(pi, pk);
                    for (size_t j = 0; j < k; ++j) v -= F[pi + Ls * j] * F[pk + Ls * j];
                    v /= lkk;
                    F[pi + Ls * k] = v;
                    dk[i] -= v * v;
                }
                rank = k + 1;
            }
            for (int32_t d = 0; d < spp; ++d) {
                const size_t base = Ls * ((size_t)d + (size_t)spp * ((size_t)s + (size_t)S * (size_t)g));
                double* o = out + base;
                for (size_t l = 0; l < Ls; ++l) o[l] = meanW[(size_t)s + (size_t)S * (l + Ls * (size_t)g)];
                for (size_t k = 0; k < rank; ++k) {
                    const double zz = z ? z[base + k]
                                        : philox_normal(seed, (1ull << 41) + (uint64_t)s + (uint64_t)S * (uint64_t)g,
                                                             (uint64_t)k + (uint64_t)L * (uint64_t)d);
                    for (size_t l = 0; l < Ls; ++l) o[l] += F[l + Ls * k] * zz;
                }
            }
        }
    return GPSLC_OK;
}

int gpslc_last_info(const gpslc_ctx* c, int32_t* info, int64_t S) {
    if (!c) return -1;
    if (!info) return -2;
    if (S != (int64_t)c->last_info.size()) return -3;
    if (S) memcpy(info, c->last_info.data(), sizeof(int32_t) * S);
    return GPSLC_OK;
}

int gpslc_profile_reset(gpslc_ctx* c) {
    if (!c) return -1;
    for (int k = 0; k < kProfClasses; ++k) { c->prof_launches[k] = 0; c->prof_ms[k] = 0; c->prof_flop[k] = 0; }
    c->prof_used = 0;
    return GPSLC_OK;
}
int gpslc_profile_get_class(gpslc_ctx* c, int32_t cls, int64_t* launches, double* total_ms, double* total_flop) {
    if (!c) return -1;
    if (cls < 0 || cls >= kProfClasses) return bad_arg(c, 2, "kernel class must be 0..4");
    if (launches) *launches = c->prof_launches[cls];
    if (total_ms) *total_ms = c->prof_ms[cls];
    if (total_flop) *total_flop = c->prof_flop[cls];
    return GPSLC_OK;
}
int gpslc_profile_get(gpslc_ctx* c, int64_t* launches, double* total_ms, double* total_flop) {
    return gpslc_profile_get_class(c, 0, launches, total_ms, total_flop);
}

}  // extern "C"
