// Host-side check of the owners of a ctx's memory (causalgpslc.jl_amd/csrc/dev_mem.h) against a fake memory policy that counts
// live blocks, live bytes and quiesce calls, keeps the order of its calls, refuses a block it does not know (double release) and
// can be told to fail the k-th allocation.  Every scenario ends with nothing live.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "../../causalgpslc.jl_amd/csrc/dev_mem.h"

static int fails = 0;
static long checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Fake {
    static std::map<void*, size_t> live;
    static size_t live_bytes;
    static long allocs, releases, quiesces, bad_releases;
    static long fail_in;          // > 0: the fail_in-th allocation from now fails
    static std::string log;       // 'Q'uiesce, 'R'elease, 'A'lloc, 'F'ailed alloc — in call order
    static void* alloc(size_t bytes) {
        if (fail_in > 0 && --fail_in == 0) { log += 'F'; return nullptr; }
        void* p = malloc(bytes ? bytes : 1);
        live[p] = bytes;
        live_bytes += bytes;
        ++allocs;
        log += 'A';
        return p;
    }
    static void release(void* p) {
        auto it = live.find(p);
        if (it == live.end()) { ++bad_releases; return; }
        live_bytes -= it->second;
        live.erase(it);
        free(p);
        ++releases;
        log += 'R';
    }
    static void quiesce() { ++quiesces; log += 'Q'; }
    static void start() { allocs = releases = quiesces = 0; fail_in = 0; log.clear(); }
    static void nothing_live(const char* where) {
        CHECK(live.empty() && live_bytes == 0 && bad_releases == 0, "%s: %zu blocks, %zu bytes live, %ld bad releases", where,
              live.size(), live_bytes, bad_releases);
    }
};
std::map<void*, size_t> Fake::live;
size_t Fake::live_bytes = 0;
long Fake::allocs = 0, Fake::releases = 0, Fake::quiesces = 0, Fake::bad_releases = 0, Fake::fail_in = 0;
std::string Fake::log;

using Buf = Buffer<Fake>;

template <class F>
static bool throws_bad_alloc(F&& f) {
    try { f(); } catch (const std::bad_alloc&) { return true; }
    return false;
}

static void buffer_reserve() {
    Fake::start();
    {
        Buf b;
        CHECK(b.data() == nullptr && b.bytes() == 0, "a new buffer is empty");
        b.reserve(0);
        CHECK(Fake::log.empty() && b.data() == nullptr, "reserve(0) on an empty buffer does nothing");
        b.reserve(1000);
        CHECK(Fake::log == "A", "first reserve: one allocation and no quiesce, got %s", Fake::log.c_str());
        CHECK(b.data() != nullptr && b.bytes() == 1000 && Fake::live_bytes == 1000, "capacity 1000");
        char* p = b.data();
        for (size_t want : {size_t(1000), size_t(999), size_t(1), size_t(0)}) {
            b.reserve(want);
            CHECK(Fake::log == "A" && b.data() == p && b.bytes() == 1000, "reserve(%zu) below the capacity changes nothing", want);
        }
        CHECK(b.as<double>() == reinterpret_cast<double*>(p) && static_cast<char*>(b) == p, "as<T>() and the conversion give the pointer");
        b.reserve(1001);
        CHECK(Fake::log == "AQRA", "growth is quiesce, release, allocate: got %s", Fake::log.c_str());
        CHECK(b.bytes() == 1001 && Fake::live.size() == 1 && Fake::live_bytes == 1001, "one block of 1001 bytes is live");
    }
    CHECK(Fake::log == "AQRAR" && Fake::quiesces == 1, "the destructor releases without a quiesce: %s", Fake::log.c_str());
    Fake::nothing_live("buffer_reserve");
}

// the progress words of a stream slot: a growth whose allocation fails must not leave a size without a pointer
static void buffer_failed_growth() {
    Fake::start();
    {
        Buf b;
        b.reserve(4096);
        Fake::fail_in = 1;
        CHECK(throws_bad_alloc([&] { b.reserve(8192); }), "a failed growth throws bad_alloc");
        CHECK(Fake::log == "AQRF", "the old block went before the failed allocation: %s", Fake::log.c_str());
        CHECK(b.data() == nullptr && b.bytes() == 0, "the buffer is empty after a failed growth");
        CHECK(Fake::live.empty() && Fake::live_bytes == 0, "nothing is live after a failed growth");
        b.reserve(4096);          // the old size again: allocates, since the capacity is 0
        CHECK(Fake::log == "AQRFA" && b.data() != nullptr && b.bytes() == 4096, "reserve of the old size allocates again: %s",
              Fake::log.c_str());
        Fake::fail_in = 1;
        Buf e;
        CHECK(throws_bad_alloc([&] { e.reserve(16); }) && e.data() == nullptr && e.bytes() == 0, "a failed first allocation leaves it empty");
        CHECK(Fake::quiesces == 1, "an empty buffer has nothing to wait for");
    }
    Fake::nothing_live("buffer_failed_growth");
}

struct Entry {        // as TaskList: plain fields and one owned block
    int key = 0;
    Buf dev;
};

static void buffer_moves() {
    Fake::start();
    {
        Buf a;
        a.reserve(100);
        char* pa = a.data();
        Buf b(std::move(a));
        CHECK(a.data() == nullptr && a.bytes() == 0, "move construction empties the source");
        CHECK(b.data() == pa && b.bytes() == 100 && Fake::live.size() == 1, "and hands the block over");
        Buf c;
        c.reserve(200);
        char* pc = c.data();
        const long rel = Fake::releases;
        b = std::move(c);
        CHECK(Fake::releases == rel + 1 && Fake::live.count(pa) == 0, "move assignment releases the destination's old block once");
        CHECK(c.data() == nullptr && c.bytes() == 0 && b.data() == pc && b.bytes() == 200, "and empties the source");
        Buf& self = b;
        b = std::move(self);
        CHECK(b.data() == pc && b.bytes() == 200 && Fake::live.size() == 1, "self-assignment keeps the block");
        a.reserve(50);            // a moved-from buffer is an empty one
        CHECK(a.bytes() == 50 && Fake::live.size() == 2, "a moved-from buffer can be used again");
        CHECK(Fake::quiesces == 0, "no move waits for anything");
    }
    Fake::nothing_live("buffer_moves");
    // the task-list cache: grown by emplace_back / push_back (reallocating), evicted by erase in the middle
    Fake::start();
    {
        std::vector<Entry> v;
        std::vector<char*> where;
        for (int i = 0; i < 9; ++i) {
            Entry e;
            e.key = i;
            e.dev.reserve(64 + (size_t)i);
            where.push_back(e.dev.data());
            if (i & 1) v.push_back(std::move(e));
            else v.emplace_back(std::move(e));
            CHECK(Fake::live.size() == v.size(), "live blocks %zu = entries %zu while growing", Fake::live.size(), v.size());
        }
        for (int i = 0; i < 9; ++i) CHECK(v[(size_t)i].dev.data() == where[(size_t)i], "entry %d kept its block across reallocation", i);
        for (size_t at : {size_t(4), size_t(0), size_t(6), size_t(2)}) {
            const int gone = v[at].key;
            v.erase(v.begin() + (long)at);
            CHECK(Fake::live.size() == v.size(), "live blocks %zu = entries %zu after erase", Fake::live.size(), v.size());
            CHECK(Fake::live.count(where[(size_t)gone]) == 0, "the erased entry's block %d is the one released", gone);
            for (const Entry& e : v)
                CHECK(e.dev.data() == where[(size_t)e.key] && e.dev.bytes() == 64 + (size_t)e.key, "entry %d still owns its own block", e.key);
        }
        v.resize(12);             // the tri_order table: resized with empty entries
        CHECK(Fake::live.size() == 5 && v[11].dev.data() == nullptr, "resize adds empty entries");
        CHECK(Fake::quiesces == 0, "vector traffic waits for nothing");
    }
    CHECK(Fake::allocs == 9 && Fake::releases == 9, "9 allocations, 9 releases: %ld, %ld", Fake::allocs, Fake::releases);
    Fake::nothing_live("vector of entries");
}

static void arena() {
    Fake::start();
    {
        Arena<Fake> a;
        CHECK(throws_bad_alloc([&] { a.take<double>(1); }) && a.off == 0, "an empty arena gives nothing");
        a.reserve(4096);
        CHECK(a.bytes() == 4096, "capacity");
        const uintptr_t base = reinterpret_cast<uintptr_t>(a.buf.data());
        std::vector<void*> first;
        const size_t counts[] = {1, 3, 32, 33, 100};
        size_t end = 0;
        for (size_t cnt : counts) {
            double* p = a.take<double>(cnt);
            const size_t o = reinterpret_cast<uintptr_t>(p) - base;
            CHECK(o % 256 == 0, "offset %zu is a multiple of 256", o);
            CHECK(o >= end && o < end + 256, "offset %zu is the first aligned one after %zu", o, end);
            end = o + cnt * sizeof(double);
            CHECK(a.off == end, "off %zu follows the piece (%zu)", a.off, end);
            first.push_back(p);
        }
        const size_t off = a.off;
        CHECK(throws_bad_alloc([&] { a.take<double>(4096 / 8); }), "a take that does not fit throws");
        CHECK(a.off == off, "and leaves off unchanged");
        const size_t room = 4096 - ((off + 255) & ~size_t(255));
        CHECK(throws_bad_alloc([&] { a.take<char>(room + 1); }) && a.off == off, "one byte too many throws");
        CHECK(a.take<char>(room) != nullptr && a.off == 4096, "what exactly fits is handed out");
        a.reset();
        CHECK(a.off == 0, "reset");
        for (size_t i = 0; i < first.size(); ++i) CHECK(a.take<double>(counts[i]) == first[i], "take %zu after reset returns the same address", i);
        a.reserve(4096);
        a.reserve(100);
        CHECK(Fake::log == "A", "arenas never shrink: %s", Fake::log.c_str());
        a.reserve(8192);
        CHECK(Fake::log == "AQRA" && a.bytes() == 8192, "arena growth is the buffer's: %s", Fake::log.c_str());
        Fake::fail_in = 1;
        CHECK(throws_bad_alloc([&] { a.reserve(1 << 20); }) && a.bytes() == 0, "a failed growth leaves capacity 0");
        a.reset();
        CHECK(throws_bad_alloc([&] { a.take<double>(1); }), "and take() refuses");
        a.reserve(512);
        CHECK(a.take<double>(64) != nullptr, "until the next reserve");
    }
    Fake::nothing_live("arena");
}

static void pool() {
    const size_t MiB = size_t(1) << 20;
    Fake::start();
    {
        PoolArena<Fake> p;
        p.reset();
        CHECK(Fake::log.empty(), "reset of an empty pool does nothing");
        // one call's takes: they overflow the first block twice
        const std::vector<size_t> seq = {0, 8, 100000, 900000, 300000, 64, 3 * MiB + 5};
        auto run = [&](std::vector<char*>& out) {
            for (size_t b : seq) out.push_back(p.take<char>(b));
        };
        std::vector<char*> got;
        run(got);
        CHECK(p.blocks.size() == 3, "three blocks chained, got %zu", p.blocks.size());
        CHECK(Fake::quiesces == 0 && Fake::releases == 0, "chaining neither waits nor frees: earlier pointers stay valid");
        for (size_t i = 0; i < got.size(); ++i) {       // every piece lies inside a live block, 256-aligned in it, none overlaps
            bool inside = false;
            for (auto& b : p.blocks) {
                const size_t need = std::max<size_t>(seq[i], 8);
                if (got[i] >= b.data() && got[i] + need <= b.data() + b.bytes()) { inside = true; CHECK((got[i] - b.data()) % 256 == 0, "piece %zu aligned", i); }
            }
            CHECK(inside, "piece %zu lies inside a live block", i);
            for (size_t j = 0; j < i; ++j)
                CHECK(got[j] + std::max<size_t>(seq[j], 8) <= got[i] || got[i] + std::max<size_t>(seq[i], 8) <= got[j], "pieces %zu and %zu overlap", j, i);
        }
        size_t total = 0;
        for (auto& b : p.blocks) { CHECK(b.bytes() >= MiB, "a chained block has at least 1 MiB, got %zu", b.bytes()); total += b.bytes(); }
        CHECK(p.blocks[2].bytes() == ((3 * MiB + 5 + 255) & ~size_t(255)), "a piece beyond 1 MiB gets a block of its own size, rounded to 256");
        CHECK(Fake::live_bytes == total, "live bytes are the chain's");
        const std::string before = Fake::log;
        p.reset();
        CHECK(Fake::log == before + "QRRRA", "reset merges: quiesce, release the chain, one allocation: %s", Fake::log.c_str());
        CHECK(p.blocks.size() == 1 && p.blocks[0].bytes() == total && Fake::live_bytes == total, "one block of the chain's total size");
        const long allocs = Fake::allocs;
        for (int round = 0; round < 3; ++round) {
            std::vector<char*> again;
            run(again);
            p.reset();
            CHECK(Fake::allocs == allocs && p.blocks.size() == 1, "round %d: the same takes allocate nothing", round);
            for (size_t i = 0; i < again.size(); ++i) CHECK(again[i] >= p.blocks[0].data() && again[i] + seq[i] <= p.blocks[0].data() + total, "piece %zu in the merged block", i);
        }
        CHECK(Fake::quiesces == 1, "a single block is reset without waiting");
        p.release();
        CHECK(p.blocks.empty() && p.off == 0 && Fake::live.empty(), "release frees everything");
        // a merge that fails leaves the pool empty and usable
        p.take<char>(MiB);
        p.take<char>(MiB);
        CHECK(p.blocks.size() == 2, "two blocks");
        Fake::fail_in = 1;
        CHECK(throws_bad_alloc([&] { p.reset(); }), "a failing merge throws");
        CHECK(p.blocks.empty() && p.off == 0 && Fake::live.empty(), "and leaves the pool empty");
        char* q = p.take<char>(10);
        CHECK(q != nullptr && p.blocks.size() == 1 && p.blocks[0].bytes() == MiB, "and usable");
        // a chained block that cannot be had: the pool keeps what it has
        Fake::fail_in = 1;
        const size_t off = p.off;
        CHECK(throws_bad_alloc([&] { p.take<char>(2 * MiB); }), "a failing chain throws");
        CHECK(p.blocks.size() == 1 && p.off == off && p.take<char>(10) > q, "and the pool goes on in its block");
    }
    Fake::nothing_live("pool");
}

int main() {
    buffer_reserve();
    buffer_failed_growth();
    buffer_moves();
    arena();
    pool();
    if (fails) { printf("FAILED %d of %ld\n", fails, checks); return 1; }
    printf("OK %ld\n", checks);
    return 0;
}
