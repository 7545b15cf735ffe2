// Ownership of a ctx's memory (host_ctx.h) as plain host C++ — no HIP in here, so that the CPU test (tests/test_dev_mem.py) compiles
// it with g++ against a counting fake.  A memory policy `Mem` says where the bytes come from:
//     static void* alloc(size_t bytes);   // null on failure
//     static void  release(void* p);
//     static void  quiesce();             // before memory that launches may still use is freed
// host_ctx.h supplies the two real ones (device memory, pinned host memory).  Every block has exactly one owner, a Buffer; an Arena
// and a PoolArena carve aligned pieces out of the Buffers they hold.
#pragma once

#include <algorithm>
#include <cstddef>
#include <new>
#include <utility>
#include <vector>

// One owned block of `Mem` memory, read as elements of T.  Move-only; freed with its owner.  The size and the pointer cannot
// disagree: this is the only place that knows either.
template <class Mem, class T = char>
class Buffer {
    void* p_ = nullptr;
    size_t bytes_ = 0;
    void drop() { if (p_) Mem::release(p_); p_ = nullptr; bytes_ = 0; }

public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) { drop(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() { drop(); }

    T* data() const { return static_cast<T*>(p_); }
    operator T*() const { return data(); }           // a Buffer stands where its pointer stood
    template <class U> U* as() const { return static_cast<U*>(p_); }
    size_t bytes() const { return bytes_; }          // capacity

    // The one growth operation: nothing if the capacity suffices; else wait for whatever may still use the old block, free it,
    // and only then allocate (the old contents are NOT kept; the two blocks never coexist).  A failed allocation leaves the
    // Buffer empty — null, capacity 0 — and throws std::bad_alloc: a later reserve starts afresh.
    void reserve(size_t bytes) {
        if (bytes_ >= bytes) return;
        if (p_) { Mem::quiesce(); drop(); }
        p_ = Mem::alloc(bytes);
        if (!p_) throw std::bad_alloc();
        bytes_ = bytes;
    }
};

// Bump allocator over one Buffer: take() hands out 256-byte-aligned pieces until reset(); it never grows by itself.
template <class Mem>
struct Arena {
    Buffer<Mem> buf;
    size_t off = 0;
    size_t bytes() const { return buf.bytes(); }
    void reserve(size_t bytes) { buf.reserve(bytes); }
    void reset() { off = 0; }
    template <class T>
    T* take(size_t count) {
        size_t a = (off + 255) & ~size_t(255);
        size_t need = count * sizeof(T);
        if (a + need > buf.bytes()) throw std::bad_alloc();
        off = a + need;
        return reinterpret_cast<T*>(buf.data() + a);
    }
};

// Growable staging pool of a ctx (host-pointer entry points: uploads, outputs, info words).  take() never moves earlier
// allocations: when the current block is full a new one is chained; the next reset() merges the chain into one block of the
// total size, so a steady-state call sequence allocates nothing.
template <class Mem>
struct PoolArena {
    std::vector<Buffer<Mem>> blocks;
    size_t off = 0;
    void release() {
        blocks.clear();
        off = 0;
    }
    void reset() {
        if (blocks.size() > 1) {
            size_t total = 0;
            for (auto& b : blocks) total += b.bytes();
            Mem::quiesce();
            release();
            add_block(total);      // a failure leaves the pool empty: the next take() starts a new chain
        }
        off = 0;
    }
    void add_block(size_t bytes) {
        Buffer<Mem> b;
        b.reserve(bytes);
        blocks.push_back(std::move(b));
        off = 0;
    }
    template <class T>
    T* take(size_t count) {
        const size_t need = std::max<size_t>(count * sizeof(T), 8);
        size_t a = (off + 255) & ~size_t(255);
        if (blocks.empty() || a + need > blocks.back().bytes()) {
            add_block(std::max<size_t>((need + 255) & ~size_t(255), size_t(1) << 20));
            a = 0;
        }
        off = a + need;
        return reinterpret_cast<T*>(blocks.back().data() + a);
    }
};
