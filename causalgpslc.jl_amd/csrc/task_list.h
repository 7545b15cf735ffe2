// Task descriptors, dependency rules and host-built task order of the persistent factorisation launch (potrf_tasks_kernel,
// k_tilegemm.hip) — plain C++ (no HIP in here): the kernel waits and publishes through task_needs / task_products, and the CPU suite
// replays the host-built order through the same two (tests/c/task_list_test.cpp: every task behind its producers in its own queue
// = the launch cannot deadlock; every tile exactly once).
#pragma once
#include <algorithm>
#include <vector>
#ifdef __HIPCC__
#define TASK_HD __host__ __device__
#else
#define TASK_HD
#endif

#define TASK_NONE 0xFFFFFFFFu
#define TASK_QUEUES 8             // one per XCD
#define TASK_LIST_HDR 32          // words of the list's header, then the descriptors
#define TASK_LIST_FIRST(q) (q)                     // header word: first descriptor of queue q
#define TASK_LIST_LEN(q) (TASK_QUEUES + (q))       // header word: descriptors of queue q
#define TASK_SYNC_HDR 32          // ints in front of the progress words ([8] unused: the time-out word is PotrfTaskArgs::timeout)
#define TASK_SYNC_HEAD(q) (q)                      // ticket head of queue q
#define TASK_SYNC_DONE 9                           // tasks finished (the measurement build's stamp slots)
#define TASK_SYNC_STRIDE 40       // progress words (ints) per matrix
#define TASK_WORD_DIAG 0                           // diagonal tiles finished
#define TASK_WORD_ROW(i) (1 + (i))                 // finished tiles of tile row i (i <= nt: the augmented row)
#define TASK_MAX_NT 32
// descriptor: bits 0..16 batch element, 17..18 number of consecutive tile rows of the column the task covers minus 1 (a diagonal
// task: 2 = it goes on with strip(k + 1, k) and, where the augmented row rides, the augmented tile (nt, k)), 19..23 column k,
// 24..29 (first) tile row i (up to nt = 32: the augmented tile row), 30..31 kind: 0 strip(i.., k), 1 diag(k), 2 unused (once a
// strip(k + 1, k) of its own that carried the augmented tile), 3 the back-substitution of the matrix
enum { TASK_STRIP = 0, TASK_DIAG = 1, TASK_BACK = 3 };
#define TASK_MAX_BATCH (1 << 17)
#define TASK_B(d) ((int)((d) & 0x1FFFF))
#define TASK_ROWS(d) ((int)(((d) >> 17) & 3) + 1)
#define TASK_K(d) ((int)(((d) >> 19) & 31))
#define TASK_I(d) ((int)(((d) >> 24) & 63))
#define TASK_KIND(d) ((int)((d) >> 30))
TASK_HD inline unsigned task_pack(int b, int k, int i, int kind, int rows = 1) {
    return (unsigned)b | ((unsigned)(rows - 1) << 17) | ((unsigned)k << 19) | ((unsigned)i << 24) | ((unsigned)kind << 30);
}

// 16-row blocks of an augmented row of `short_rows` right-hand sides that ride with the diagonal tasks (potrf_tasks_kernel's MT:
// 1 or 2); 0: more than 32 right-hand sides, the row is an ordinary tile row of the list (build_task_list's aug_full)
inline int task_aug_blocks(int short_rows) { return short_rows > 32 ? 0 : (short_rows + 15) / 16; }

// ---- the dependency rules, stated once for the kernel and the CPU replay: a task may start when every need(word, value) holds
// as "progress word `word` of its matrix >= value", and having finished it sets every put(word, value), one call per word.
// aug_rides: the augmented row's tiles ride with the diagonal tasks (the kernel's MT > 0).
template <class F>
TASK_HD inline void task_needs(unsigned d, int nt, bool aug_rides, F&& need) {
    const int kind = TASK_KIND(d), k = TASK_K(d), i = TASK_I(d), rows = TASK_ROWS(d);
    if (kind == TASK_BACK) {            // the whole factor and the solved augmented row
        need(TASK_WORD_DIAG, nt);
        need(TASK_WORD_ROW(nt), nt);
    } else if (kind == TASK_DIAG) {     // tile row k (and the riding augmented row) final up to column k - 1
        if (k > 0) {
            need(TASK_WORD_ROW(k), k);
            if (aug_rides) need(TASK_WORD_ROW(nt), k);
            if (rows > 1) need(TASK_WORD_ROW(k + 1), k);      // ... and tile row k + 1 for the strip it goes on with
        }
    } else {                            // strip(i.., k): inv(L_kk) and tile row k (diag(k)), its tile rows up to column k - 1
        need(TASK_WORD_DIAG, k + 1);
        // a riding augmented row (i == nt) has its column update from diag(k); as an ordinary tile row it carries its own
        if ((i < nt || !aug_rides) && k > 0)
            for (int r = 0; r < rows; ++r) need(TASK_WORD_ROW(i + r), k);
    }
}
template <class F>
TASK_HD inline void task_products(unsigned d, int nt, bool aug_rides, F&& put) {
    const int kind = TASK_KIND(d), k = TASK_K(d), i = TASK_I(d), rows = TASK_ROWS(d);
    if (kind == TASK_DIAG) {
        put(TASK_WORD_DIAG, k + 1);
        if (rows > 1) {                 // strip(k + 1, k) and the riding augmented tile (nt, k): what diag(k + 1) waits for
            put(TASK_WORD_ROW(k + 1), k + 1);
            if (aug_rides) put(TASK_WORD_ROW(nt), k + 1);
        }
    } else if (kind == TASK_STRIP)
        for (int r = 0; r < rows; ++r) put(TASK_WORD_ROW(i + r), k + 1);
    // back: nobody in the launch reads alpha
}

// ---- the persistent factorisation launch (potrf_tasks_kernel, k_tilegemm.hip) -------------------------------------------
// Task order of one queue (= one XCD's contiguous run of matrices).  Stages of a matrix: s = 2k: diag(k), s = 2k + 1: the
// strips of column k.  Matrices are taken in groups of G; step t of the order holds stage s of group t - s for every s — a
// skewed wavefront, so that (1) every task follows its producers (stage s - 1 of the same group sits one whole step
// earlier: ~ G * (nt + nt (nt + 1) / 2) tickets, several rounds of the XCD's 64 workgroup slots — a consumer practically
// never finds its producer unfinished), and (2) every stretch of the order mixes the latency-bound diagonal tasks of some
// groups with the MFMA-bound strips of others.  Inside a stage the strips of one matrix are consecutive tickets: they run
// at the same time on one XCD and share the B panel L(k, 0..k-1) in its L2.
inline std::vector<unsigned> build_task_list(int nt, int back, int nb, int G, int rows_per_task, bool aug_full, long long* ntasks_out) {
    std::vector<unsigned> out(TASK_LIST_HDR, 0u);
    const int NS = 2 * nt + (back ? 1 : 0);       // back: one more stage, the back-substitution of the finished factor
    long long total = 0;
    const int wq = nb / TASK_QUEUES, wrm = nb % TASK_QUEUES;
    for (int x = 0; x < TASK_QUEUES; ++x) {
        const int x0 = x * wq + std::min(x, wrm), xc = wq + (x < wrm ? 1 : 0);
        const size_t first = out.size() - TASK_LIST_HDR;
        const int NG = (xc + G - 1) / G;
        for (int t = 0; t < NG + NS - 1; ++t)
            for (int s = 0; s < NS; ++s) {
                const int g = t - s;
                if (g < 0 || g >= NG) continue;
                const int k = s >> 1;
                for (int j = g * G; j < std::min(xc, (g + 1) * G); ++j) {
                    const int b = x0 + j;
                    if (s == 2 * nt) { out.push_back(task_pack(b, 0, 0, TASK_BACK)); continue; }
                    // a diagonal task goes on with the strip of tile row k + 1 and the riding augmented tile of its column (rows = 2
                    // in its descriptor); the last column has no such strip: its augmented tile is a task of its own
                    if ((s & 1) == 0) { out.push_back(task_pack(b, k, k, TASK_DIAG, k + 1 < nt ? 2 : 1)); continue; }
                    // aug_full (more than 32 right-hand sides): the augmented row is a tile row like the others, strip(nt, k) in
                    // every column; otherwise its tiles ride with the diagonal tasks and only the last column's is a task of its own
                    if (aug_full || k + 1 == nt) out.push_back(task_pack(b, k, nt, TASK_STRIP));
                    for (int i = k + 2; i < nt; i += rows_per_task)
                        out.push_back(task_pack(b, k, i, TASK_STRIP, std::min(rows_per_task, nt - i)));
                }
            }
        out[TASK_LIST_FIRST(x)] = (unsigned)first;
        out[TASK_LIST_LEN(x)] = (unsigned)(out.size() - TASK_LIST_HDR - first);
        total += out[TASK_LIST_LEN(x)];
    }
    *ntasks_out = total;
    return out;
}

