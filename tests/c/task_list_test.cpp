// Host-side check of the task order of the persistent factorisation launch (causalgpslc.jl_amd/csrc/task_list.h).  The replay
// runs on task_needs / task_products, the functions potrf_tasks_kernel (k_tilegemm.hip) itself waits and publishes through.
// Inside a queue tickets are handed out in list order to RUNNING workgroups, so "every producer of a task sits EARLIER in the
// task's own queue" is the whole no-deadlock argument: replaying each queue sequentially, every need must already hold after
// the tasks before it.  Also: a matrix lives in exactly one queue, every progress word moves exactly once per column and column
// by column, the right-hand-side row ends complete.
// That the shared rules are SUFFICIENT is checked against this file's own statement of the left-looking algorithm, in tiles
// (tile_reads below): tables of final tiles, driven by the products, must hold every tile a task reads — the table of what the
// replay has produced so far, and the table of what the task KNOWS to be final: the tiles behind the publishes its needs name,
// and behind the needs of those tasks in turn.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>
#include "../../causalgpslc.jl_amd/csrc/task_list.h"

static int fails = 0;
static bool quiet = false;      // the broken lists below: count the violations, do not print them
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20 && !quiet) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// Tile (i, j) of a matrix, j <= i, i = nt: the augmented row (its diagonal tile does not exist).  What a task READS, from the
// left-looking factorisation L(i, k) = (A(i, k) - sum_{j < k} L(i, j) L(k, j)^T) inv(L(k, k))^T, not from the progress words:
// read(i, j0, j1) = the tiles (i, j0 .. j1 - 1)
template <class F>
static void tile_reads(int kind, int k, int i, int rows, int nt, bool aug_rides, F&& read) {
    if (kind == TASK_BACK) {                    // the whole factor and the solved right-hand sides
        for (int r = 0; r <= nt; ++r) read(r, 0, std::min(r + 1, nt));
    } else if (kind == TASK_DIAG) {             // A(k, k) - sum_j L(k, j) L(k, j)^T, the riding augmented tile (nt, k) likewise
        read(k, 0, k);
        if (aug_rides) read(nt, 0, k);
        if (rows > 1) read(k + 1, 0, k);        // it goes on with strip(k + 1, k): its own tile (k, k) is in hand
    } else {
        for (int r = i; r < i + rows; ++r) read(r, 0, k);
        read(k, 0, k + 1);                      // (k, k) with its inverse, which diag(k) writes with it
    }
}

// replays list L; returns the number of violations it found
static int replay(const std::vector<unsigned>& L, long long ntasks, int nt, int nb, int back, bool aug_full) {
    const int fails0 = fails;
    const bool aug_rides = !aug_full;
    CHECK((long long)L.size() == TASK_LIST_HDR + ntasks, "size");
    std::vector<int> prog((size_t)nb * TASK_SYNC_STRIDE, 0), queue_of(nb, -1), backs(nb, 0);
    // tables of final tiles, one word per tile row (bit j = tile (i, j)): final[b * TW + i] = what the replay has produced so far;
    // known[((b * (nt + 2) + word) * TW + value) * TW + i] = what is final for whoever sees progress word `word` at `value`
    const int TW = nt + 1;
    const bool deep = nb <= 9;      // the second table for the small batches only (the rules do not depend on the count): run time
    std::vector<uint32_t> final((size_t)nb * TW, 0), known(deep ? (size_t)nb * (nt + 2) * TW * TW : 0, 0), mine(TW);
    long long seen = 0;
    for (int x = 0; x < TASK_QUEUES; ++x) {
        const unsigned first = L[TASK_LIST_FIRST(x)], len = L[TASK_LIST_LEN(x)];
        for (unsigned t = 0; t < len; ++t, ++seen) {
            if (TASK_LIST_HDR + (size_t)first + t >= L.size()) { CHECK(false, "queue %d runs past the list", x); break; }
            const unsigned d = L[TASK_LIST_HDR + first + t];
            const int b = TASK_B(d), k = TASK_K(d), i = TASK_I(d), r = TASK_ROWS(d), kind = TASK_KIND(d);
            CHECK(b >= 0 && b < nb, "matrix index %d", b);
            if (b < 0 || b >= nb) continue;
            CHECK(queue_of[b] == -1 || queue_of[b] == x, "matrix %d in queues %d and %d", b, queue_of[b], x);
            queue_of[b] = x;
            CHECK(kind == TASK_BACK || kind == TASK_DIAG || kind == TASK_STRIP, "kind %d", kind);
            if (kind == TASK_BACK) { CHECK(back, "back task without back"); ++backs[b]; }
            else if (kind == TASK_DIAG) CHECK(r == 1 || (r == 2 && k + 1 < nt), "diag(%d,%d) covers %d rows", b, k, r);
            else CHECK(i + r - 1 <= nt && i > k, "strip rows %d..%d of column %d", i, i + r - 1, k);
            int* p = &prog[(size_t)b * TASK_SYNC_STRIDE];
            uint32_t* fin = &final[(size_t)b * TW];
            // the kernel's wait: every need holds after the tasks before this one
            task_needs(d, nt, aug_rides, [&](int word, int value) {
                CHECK(p[word] >= value, "task %08x (matrix %d kind %d k %d i %d): word %d at %d, needs %d", d, b, kind, k, i, word, p[word], value);
            });
            // ... and the needs cover every tile the task reads: final in the replay's order
            tile_reads(kind, k, i, r, nt, aug_rides, [&](int ti, int j0, int j1) {
                const uint32_t cols = (uint32_t)((1ull << j1) - (1ull << j0));
                CHECK((fin[ti] & cols) == cols, "task %08x (matrix %d kind %d k %d i %d) reads tiles (%d,%d..%d) before they are final: %08x", d, b, kind, k, i,
                      ti, j0, j1 - 1, fin[ti]);
            });
            // ... and known to be final through the needs (workgroups run tasks concurrently: a tile that merely sits earlier in
            // the list is not a tile the task may read)
            uint32_t* kn = deep ? &known[(size_t)b * (nt + 2) * TW * TW] : nullptr;
            if (deep) {
                std::fill(mine.begin(), mine.end(), 0u);
                task_needs(d, nt, aug_rides, [&](int word, int value) {
                    for (int w = 0; w < TW; ++w) mine[w] |= kn[((size_t)word * TW + value) * TW + w];
                });
                tile_reads(kind, k, i, r, nt, aug_rides, [&](int ti, int j0, int j1) {
                    const uint32_t cols = (uint32_t)((1ull << j1) - (1ull << j0));
                    CHECK((mine[ti] & cols) == cols, "task %08x (matrix %d kind %d k %d i %d) reads tiles (%d,%d..%d), which its needs do not make final: %08x",
                          d, b, kind, k, i, ti, j0, j1 - 1, mine[ti]);
                });
            }
            // the kernel's publish: each word exactly once per column, column by column
            task_products(d, nt, aug_rides, [&](int word, int value) {
                CHECK(p[word] == value - 1, "task %08x (matrix %d kind %d k %d i %d): word %d out of order: %d -> %d", d, b, kind, k, i, word, p[word], value);
                p[word] = value;
                const int ti = word == TASK_WORD_DIAG ? value - 1 : word - TASK_WORD_ROW(0);
                fin[ti] |= 1u << (value - 1);
                if (deep) mine[ti] |= 1u << (value - 1);
            });
            if (deep)
                task_products(d, nt, aug_rides, [&](int word, int value) { std::copy(mine.begin(), mine.end(), kn + ((size_t)word * TW + value) * TW); });
        }
    }
    CHECK(seen == ntasks, "task count");
    for (int b = 0; b < nb; ++b) {
        const int* p = &prog[(size_t)b * TASK_SYNC_STRIDE];
        CHECK(queue_of[b] >= 0, "matrix %d has no tasks", b);
        CHECK(p[TASK_WORD_DIAG] == nt, "matrix %d: %d diagonal tiles", b, p[TASK_WORD_DIAG]);
        for (int i = 1; i < nt; ++i) CHECK(p[TASK_WORD_ROW(i)] == i, "matrix %d row %d: %d tiles", b, i, p[TASK_WORD_ROW(i)]);
        CHECK(p[TASK_WORD_ROW(nt)] == nt, "matrix %d: augmented row at %d", b, p[TASK_WORD_ROW(nt)]);
        CHECK(backs[b] == (back ? 1 : 0), "matrix %d: %d back tasks", b, backs[b]);
        for (int i = 0; i <= nt; ++i)
            CHECK(final[(size_t)b * TW + i] == (uint32_t)((1ull << std::min(i + 1, nt)) - 1), "matrix %d: tile row %d ends at %08x", b, i, final[(size_t)b * TW + i]);
    }
    return fails - fails0;
}

static void run(int nt, int nb, int G, int rows, int back, bool aug_full) {
    long long ntasks = 0;
    const std::vector<unsigned> L = build_task_list(nt, back, nb, G, rows, aug_full, &ntasks);
    replay(L, ntasks, nt, nb, back, aug_full);
}

// ---- the replay has teeth: a valid list, broken on purpose, must be flagged --------------------------------------------------
typedef std::vector<std::vector<unsigned>> Queues;
static Queues split(const std::vector<unsigned>& L) {
    Queues q(TASK_QUEUES);
    for (int x = 0; x < TASK_QUEUES; ++x)
        q[x].assign(L.begin() + TASK_LIST_HDR + L[TASK_LIST_FIRST(x)], L.begin() + TASK_LIST_HDR + L[TASK_LIST_FIRST(x)] + L[TASK_LIST_LEN(x)]);
    return q;
}
static std::vector<unsigned> join(const Queues& q) {
    std::vector<unsigned> L(TASK_LIST_HDR, 0u);
    for (int x = 0; x < TASK_QUEUES; ++x) {
        L[TASK_LIST_FIRST(x)] = (unsigned)(L.size() - TASK_LIST_HDR);
        L[TASK_LIST_LEN(x)] = (unsigned)q[x].size();
        L.insert(L.end(), q[x].begin(), q[x].end());
    }
    return L;
}
static size_t find_task(const std::vector<unsigned>& q, int b, int kind, int k, int row) {      // row < 0: any
    for (size_t t = 0; t < q.size(); ++t) {
        const unsigned d = q[t];
        if (TASK_B(d) == b && TASK_KIND(d) == kind && TASK_K(d) == k && (row < 0 || (TASK_I(d) <= row && row < TASK_I(d) + TASK_ROWS(d)))) return t;
    }
    return q.size();
}

static void broken_lists_are_flagged(int nt, int nb, int G, int rows, int back, bool aug_full) {
    long long ntasks = 0;
    const std::vector<unsigned> L = build_task_list(nt, back, nb, G, rows, aug_full, &ntasks);
    CHECK(replay(join(split(L)), ntasks, nt, nb, back, aug_full) == 0 && join(split(L)) == L, "split / join changes a valid list");
    const int b = 0, k = 2;                 // matrix 0 sits in queue 0; diag(2) goes on with strip(3, 2): it needs strip(3.., 1)
    const Queues Q = split(L);
    const int before = fails;
    quiet = true;
    int flagged[4];
    {   // a diagonal task moved in front of a strip it needs
        Queues q = Q;
        const size_t s = find_task(q[0], b, TASK_STRIP, k - 1, k + 1), dg = find_task(q[0], b, TASK_DIAG, k, -1);
        if (s < dg && dg < q[0].size()) {
            const unsigned d = q[0][dg];
            q[0].erase(q[0].begin() + (long)dg);
            q[0].insert(q[0].begin() + (long)s, d);
        }
        flagged[0] = (s < dg && dg < q[0].size()) ? replay(join(q), ntasks, nt, nb, back, aug_full) : 0;
    }
    {   // a descriptor dropped: that strip (the list's count corrected, so that the rules must notice, not the length)
        Queues q = Q;
        const size_t s = find_task(q[0], b, TASK_STRIP, k - 1, k + 1);
        if (s < q[0].size()) q[0].erase(q[0].begin() + (long)s);
        flagged[1] = replay(join(q), ntasks - 1, nt, nb, back, aug_full);
    }
    {   // ... and a diagonal task dropped
        Queues q = Q;
        const size_t dg = find_task(q[0], b, TASK_DIAG, k, -1);
        if (dg < q[0].size()) q[0].erase(q[0].begin() + (long)dg);
        flagged[2] = replay(join(q), ntasks - 1, nt, nb, back, aug_full);
    }
    {   // one matrix's tasks split over two queues: the tail of queue 0 (the last tasks of its last matrix) goes to queue 1
        Queues q = Q;
        const size_t cut = q[0].size() - 2;
        q[1].insert(q[1].end(), q[0].begin() + (long)cut, q[0].end());
        q[0].resize(cut);
        flagged[3] = replay(join(q), ntasks, nt, nb, back, aug_full);
    }
    quiet = false;
    fails = before;
    const char* what[4] = {"diagonal task in front of a strip it needs", "strip dropped", "diagonal task dropped", "matrix split over two queues"};
    for (int m = 0; m < 4; ++m)
        CHECK(flagged[m] > 0, "broken list not flagged (%s): nt %d nb %d G %d rows %d back %d aug_full %d", what[m], nt, nb, G, rows, back, (int)aug_full);
}

int main() {
    int n = 0;
    const int nbs[] = {1, 3, 7, 8, 9, 64, 125, 1000}, Gs[] = {1, 3, 8, 32, 64, 4096};
    for (int nt = 2; nt <= TASK_MAX_NT; ++nt) for (int nb : nbs) for (int G : Gs) for (int rows = 1; rows <= 4; ++rows)
        for (int back = 0; back < 2; ++back) for (int aug = 0; aug < 2; ++aug) {
            if (nb == 1000 && (nt > 9 || rows > 2)) continue;      // keep the run short
            run(nt, nb, G, rows, back, aug != 0);
            ++n;
        }
    for (int nt : {4, 9, 32}) for (int nb : {16, 125}) for (int G : {1, 32}) for (int rows = 1; rows <= 2; ++rows)
        for (int back = 0; back < 2; ++back) for (int aug = 0; aug < 2; ++aug) broken_lists_are_flagged(nt, nb, G, rows, back, aug != 0);
    // descriptor fields at their limits
    const unsigned d = task_pack(TASK_MAX_BATCH - 1, 31, 32, TASK_STRIP, 4);
    CHECK(TASK_B(d) == TASK_MAX_BATCH - 1 && TASK_K(d) == 31 && TASK_I(d) == 32 && TASK_ROWS(d) == 4 && TASK_KIND(d) == TASK_STRIP, "pack");
    CHECK(TASK_KIND(task_pack(TASK_MAX_BATCH - 1, 31, 31, TASK_BACK, 4)) == TASK_BACK && TASK_KIND(task_pack(0, 0, 0, TASK_DIAG)) == TASK_DIAG, "kind");
    CHECK(TASK_SYNC_STRIDE >= TASK_WORD_ROW(TASK_MAX_NT) + 1, "progress words");
    CHECK(TASK_LIST_HDR >= TASK_LIST_LEN(TASK_QUEUES - 1) + 1 && TASK_SYNC_HDR > TASK_SYNC_DONE && TASK_SYNC_DONE > TASK_SYNC_HEAD(TASK_QUEUES - 1), "headers");
    CHECK(task_aug_blocks(1) == 1 && task_aug_blocks(16) == 1 && task_aug_blocks(17) == 2 && task_aug_blocks(32) == 2 && task_aug_blocks(33) == 0 &&
          task_aug_blocks(128) == 0, "augmented-row blocks");
    printf("%s %d\n", fails ? "FAILED" : "OK", n);
    return fails ? 1 : 0;
}
