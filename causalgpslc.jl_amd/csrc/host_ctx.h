// The bottom layer of the library's host side: the context (struct gpslc_ctx), the owners of its HIP resources, the error
// plumbing (HC, guarded) and the declarations of the utilities api.hip defines on nothing but a context.  Host only.  Every
// other host file sees a ctx through this header; it knows nothing of schedules, prediction calls or entry points.
#pragma once
#include "../../include/gpslc_hip.h"
#include "gpslc_internal.h"
#include "dev_mem.h"

#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

// what the host files share lives in this namespace: none of it (up, gemm, loo, ...) is a global symbol of the library
namespace gpslc_host {

struct HipFail {
    hipError_t e;
    const char* what;
    const char* file;
    int line;
};
#define HC(x)                                                         \
    do {                                                              \
        hipError_t _e = (x);                                          \
        if (_e != hipSuccess) throw HipFail{_e, #x, __FILE__, __LINE__}; \
    } while (0)

// a call whose workspace cannot fit, with a message that says what was too large (guarded: GPSLC_ERR_NOMEM with this text)
struct WorkspaceTooLarge : std::bad_alloc {
    std::string msg;
    explicit WorkspaceTooLarge(std::string m) : msg(std::move(m)) {}
    const char* what() const noexcept override { return msg.c_str(); }
};

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

}  // namespace gpslc_host
// the public header names struct gpslc_ctx, so it is global; this header is private to the library's host sources, which all
// work in terms of the namespace's names
using namespace gpslc_host;

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

namespace gpslc_host {

// defined in api.hip
void set_err(gpslc_ctx* c, const std::string& s);
int fail_hip(gpslc_ctx* c, const HipFail& f);
int bad_arg(gpslc_ctx* c, int k, const char* what);
void ensure_streams(gpslc_ctx* c);
double* up(DevBuffer<double>& b, const double* host, size_t count);
double* up(gpslc_ctx* c, const double* host, size_t count);
void copy_out_rows(gpslc_ctx* c, void* dst, size_t dpitch, const void* src_dev, size_t row_bytes, size_t rows);
void copy_out_large(gpslc_ctx* c, void* dst, const void* src_dev, size_t bytes);
int first_info(const gpslc_ctx* c);
void prof_collect(gpslc_ctx* c);

template <class F>
int guarded(gpslc_ctx* c, F&& f) {
    try {
        if (c) HC(hipSetDevice(c->device));
        return f();
    } catch (const HipFail& h) {
        return fail_hip(c, h);
    } catch (const WorkspaceTooLarge& w) {
        set_err(c, w.msg);
        return GPSLC_ERR_NOMEM;
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

}  // namespace gpslc_host
