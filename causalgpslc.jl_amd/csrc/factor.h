// The scheduling layer under a prediction call: the profiled tile launch and the three factorisation schedules (panels, robust,
// the persistent task launch).  It works on a ctx, a stream slot and tile references; it knows nothing of posterior samples,
// levels, chunks or entry points.
#pragma once
#include "host_ctx.h"
#include "tile_launch.h"

#include <cstdio>
#include <memory>
#include <vector>

namespace gpslc_host {

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

void rearm_queue(StreamSlot& s);
GemmArgs on_slot(GemmArgs g, const StreamSlot& s);
void gemm(gpslc_ctx* c, const GemmArgs& g0, StreamSlot& s, int prof_base);
const unsigned short* tri_order(gpslc_ctx* c, int m);
bool potrf_tasks_ok(const gpslc_ctx* c, int nt, int ntot, int short_rows, bool skip_aug_diag, int nb, const double* inv);
void potrf_tasks(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, double* inv, int* info, int info_base, int nb, int short_rows,
                 double* back_alpha);
void check_task_timeout(gpslc_ctx* c);
void reset_stale_task_timeouts(gpslc_ctx* c);
void factor_robust(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, int* info, int info_base, int nb, int prof_base);
void factor_panels(gpslc_ctx* c, StreamSlot& s, const TRef& M, int nt, int ntot, double* inv, int* info, int info_base, int nb,
                   int aug_rows, bool skip_aug_diag, int prof_base);

}  // namespace gpslc_host
