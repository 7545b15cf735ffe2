// libgpslc_hip.so, host side: the context and the utilities that need nothing but a context (host_ctx.h declares them for the
// layers above: factor.hip, predict.hip, api_predict.hip, api_score.hip), and the entry points of include/gpslc_hip.h that need
// no more than those: create / destroy, data and tuning, errors, profiling, the element-wise kernels, the summaries.  No
// exception crosses the ABI (everything is caught and mapped to a status code); every HIP error is reported through
// gpslc_last_error.
#include "host_ctx.h"
#include "philox.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

namespace gpslc_host {

void set_err(gpslc_ctx* c, const std::string& s) {
    if (c) c->err = s;
}

int fail_hip(gpslc_ctx* c, const HipFail& f) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d in `%s`", (int)f.e, hipGetErrorString(f.e), f.file,
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

int first_info(const gpslc_ctx* c) {
    for (int32_t v : c->last_info)
        if (v != 0) return v;
    return 0;
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

}  // namespace gpslc_host

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
