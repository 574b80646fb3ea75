// DevMem<T>: the one owner of a device allocation of the engine (PinMem<T>: of a page-locked host one).  Move-only; the pointer and
// its size in bytes travel together, a failed allocation leaves the object empty, and the destructor releases: no release list to
// keep in step with a struct, no early return that skips a free.  Host-only and free of HIP: allocation goes through the hooks
// below, which engine.cpp defines over the HIP runtime (and counts: pa_device_bytes_live) and tests/device_mem_main.cpp over malloc.
// A destructor frees at once: whoever lets one run has waited for the work that uses the buffer.
#pragma once
#include <cassert>
#include <cstddef>
#include <utility>

int dev_alloc(void** p, size_t bytes);      // 0, or the runtime's error code (*p is then not used)
void dev_free(void* p, size_t bytes);
int pin_alloc(void** p, size_t bytes);      // page-locked host memory, likewise
void pin_free(void* p, size_t bytes);

template <class T, bool Pinned = false>
class DevMem {
public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~DevMem() { reset(); }      // (the move operations above leave no copy operations)

    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) Pinned ? pin_free(p_, bytes_) : dev_free(p_, bytes_);
        p_ = nullptr; bytes_ = 0;
    }
    // an empty buffer gets `bytes`; returns the hook's code and stays empty when that is not 0
    int alloc(size_t bytes) {
        assert(!p_);
        void* q = nullptr;
        const int r = Pinned ? pin_alloc(&q, bytes) : dev_alloc(&q, bytes);
        if (r == 0) { p_ = static_cast<T*>(q); bytes_ = bytes; }
        return r;
    }
    // grow on demand: nothing to do while bytes() >= need, else the old buffer goes (its contents with it) and `alloc_bytes`, the
    // caller's growth policy, are allocated; empty on failure
    int fit(size_t need, size_t alloc_bytes) {
        if (bytes_ >= need) return 0;
        reset();
        return alloc(alloc_bytes);
    }
    // ... keeping the first `keep` bytes: copy(dst, src, n) -> 0 | error moves them into the new buffer before the old one goes; a
    // failed allocation or copy leaves the old buffer as it was
    template <class Copy> int fit_keep(size_t need, size_t alloc_bytes, size_t keep, Copy copy) {
        if (bytes_ >= need) return 0;
        DevMem fresh;
        int r = fresh.alloc(alloc_bytes);
        if (r == 0 && p_ && keep) r = copy(fresh.p_, p_, keep);
        if (r == 0) *this = std::move(fresh);
        return r;
    }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

template <class T> using PinMem = DevMem<T, true>;
