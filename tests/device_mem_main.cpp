// csrc/device_mem.h on the CPU (tests/test_device_mem_host.py): the hooks over malloc / free, with counters and a switch that makes
// the k-th allocation from now fail.  Every scenario starts from cleared counters and prints one line "name key=value ...", read by
// the test; `live` is the hooks' own sum of allocated minus freed bytes, `bad_free` a free of something that is not allocated
// (a second free of the same buffer among them), `old_freed` / `new_freed` how often one particular allocation was freed.
#include "device_mem.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace {
struct Counters {
    long allocs = 0, frees = 0, failed = 0, bad_free = 0, attempts = 0, fail_at = 0;
    long frees_at_last_alloc = -1;
    size_t live = 0, last_alloc_bytes = 0;
    std::map<void*, int> id_of;          // live allocations -> their number (addresses are reused, numbers are not)
    std::vector<int> freed_times;        // allocation number -> frees of it
};
Counters dev, pin;

int hook_alloc(Counters& c, void** p, size_t bytes) {
    if (++c.attempts == c.fail_at) { ++c.failed; return 2; }          // (2: what the runtime says when it is out of memory)
    *p = malloc(bytes ? bytes : 1);
    c.id_of[*p] = (int)c.freed_times.size();
    c.freed_times.push_back(0);
    c.frees_at_last_alloc = c.frees;
    ++c.allocs; c.live += bytes; c.last_alloc_bytes = bytes;
    return 0;
}
void hook_free(Counters& c, void* p, size_t bytes) {
    auto it = c.id_of.find(p);
    if (it == c.id_of.end()) { ++c.bad_free; return; }
    ++c.freed_times[(size_t)it->second];
    c.id_of.erase(it);
    free(p);
    ++c.frees; c.live -= bytes;
}
int id_of(const void* p) { auto it = dev.id_of.find(const_cast<void*>(p)); return it == dev.id_of.end() ? -1 : it->second; }
int freed(int id) { return id < 0 ? -1 : dev.freed_times[(size_t)id]; }

void scenario(const char* name) { dev = Counters{}; pin = Counters{}; printf("%s", name); }
void kv(const char* k, long long v) { printf(" %s=%lld", k, v); }
void counters() {          // after the scenario's objects are gone: ends its line
    kv("allocs", dev.allocs); kv("frees", dev.frees); kv("failed", dev.failed); kv("bad_free", dev.bad_free);
    kv("live", (long long)dev.live); kv("last_alloc_bytes", (long long)dev.last_alloc_bytes);
    kv("pin_allocs", pin.allocs); kv("pin_frees", pin.frees); kv("pin_live", (long long)pin.live);
    printf("\n");
}
int copy_ok(void* dst, const void* src, size_t n) { memcpy(dst, src, n); return 0; }
int copy_fails(void*, const void*, size_t) { return 7; }
void fill(unsigned char* p, size_t n, unsigned seed) { for (size_t i = 0; i < n; ++i) p[i] = (unsigned char)(seed + 31 * i); }
long same(const unsigned char* p, size_t n, unsigned seed) {
    for (size_t i = 0; i < n; ++i) if (p[i] != (unsigned char)(seed + 31 * i)) return 0;
    return 1;
}

struct Several {          // the shape of the engine's Lane: owners among plain members, released by `s = Several{}`
    int tag = 0;
    DevMem<char> a;
    std::vector<int> v;
    DevMem<int> b;
    DevMem<float> c;
};
}  // namespace

int dev_alloc(void** p, size_t bytes) { return hook_alloc(dev, p, bytes); }
void dev_free(void* p, size_t bytes) { hook_free(dev, p, bytes); }
int pin_alloc(void** p, size_t bytes) { return hook_alloc(pin, p, bytes); }
void pin_free(void* p, size_t bytes) { hook_free(pin, p, bytes); }

int main() {
    scenario("alloc_then_destroy");
    {
        DevMem<char> m;
        kv("empty_null", m.get() == nullptr && m.bytes() == 0 && !m);
        kv("r", m.alloc(100)); kv("bytes", (long long)m.bytes()); kv("nonnull", m.get() != nullptr && (bool)m);
        kv("live_inside", (long long)dev.live); kv("frees_inside", dev.frees);
    }
    counters();

    scenario("reset_twice");
    {
        DevMem<char> m;
        m.alloc(10); m.reset(); m.reset();
        kv("null", m.get() == nullptr); kv("bytes", (long long)m.bytes());
    }
    counters();

    scenario("fit_below_capacity");
    {
        DevMem<char> m;
        m.alloc(100);
        char* p = m.get();
        kv("r", m.fit(60, 999)); kv("r_equal", m.fit(100, 999)); kv("same_ptr", m.get() == p); kv("bytes", (long long)m.bytes());
        kv("allocs_inside", dev.allocs); kv("frees_inside", dev.frees);
    }
    counters();

    scenario("fit_above_capacity");
    {
        DevMem<char> m;
        m.alloc(100);
        const int old = id_of(m.get());
        kv("r", m.fit(101, 250)); kv("bytes", (long long)m.bytes()); kv("nonnull", m.get() != nullptr);
        kv("allocs_inside", dev.allocs); kv("frees_inside", dev.frees); kv("old_freed", freed(old));
        kv("freed_before_alloc", dev.frees_at_last_alloc == 1); kv("live_inside", (long long)dev.live);
    }
    counters();

    scenario("fit_from_empty");
    {
        DevMem<int> m;
        kv("r0", m.fit(0, 64)); kv("allocs_after_fit0", dev.allocs);
        kv("r", m.fit(40, 64)); kv("bytes", (long long)m.bytes());
    }
    counters();

    scenario("alloc_fails");
    {
        DevMem<char> m;
        dev.fail_at = 1;
        kv("r", m.alloc(100)); kv("null", m.get() == nullptr && !m); kv("bytes", (long long)m.bytes());
        kv("r_again", m.alloc(30)); kv("bytes_again", (long long)m.bytes());          // the object is usable afterwards
    }
    counters();

    scenario("fit_fails");          // stage_frames / d_stage: no pointer is left behind with a capacity
    {
        DevMem<char> m;
        m.alloc(100);
        const int old = id_of(m.get());
        dev.fail_at = dev.attempts + 1;
        kv("r", m.fit(200, 400)); kv("null", m.get() == nullptr && !m); kv("bytes", (long long)m.bytes());
        kv("old_freed", freed(old)); kv("frees_inside", dev.frees); kv("live_inside", (long long)dev.live);
    }
    counters();

    scenario("keep_prefix");
    {
        DevMem<unsigned char> m;
        m.alloc(64);
        fill(m.get(), 64, 5);
        const int old = id_of(m.get());
        kv("r_below", m.fit_keep(64, 256, 40, copy_fails)); kv("allocs_below", dev.allocs);          // nothing to do: no copy either
        kv("r", m.fit_keep(65, 256, 40, copy_ok)); kv("bytes", (long long)m.bytes()); kv("prefix_same", same(m.get(), 40, 5));
        kv("old_freed", freed(old)); kv("frees_inside", dev.frees); kv("allocs_inside", dev.allocs); kv("live_inside", (long long)dev.live);
    }
    counters();

    scenario("keep_prefix_from_empty");
    {
        DevMem<unsigned char> m;
        kv("r", m.fit_keep(10, 32, 0, copy_fails)); kv("bytes", (long long)m.bytes());          // nothing to keep: copy is not called
    }
    counters();

    scenario("keep_prefix_copy_fails");          // grow: the new buffer must not leak, the old one stays
    {
        DevMem<unsigned char> m;
        m.alloc(64);
        fill(m.get(), 64, 9);
        unsigned char* p = m.get();
        const int old = id_of(p);
        kv("r", m.fit_keep(128, 256, 40, copy_fails)); kv("same_ptr", m.get() == p); kv("bytes", (long long)m.bytes());
        kv("contents_same", same(m.get(), 64, 9)); kv("old_freed", freed(old)); kv("new_freed", freed(old + 1));
        kv("allocs_inside", dev.allocs); kv("frees_inside", dev.frees); kv("live_inside", (long long)dev.live);
    }
    counters();

    scenario("keep_prefix_alloc_fails");
    {
        DevMem<unsigned char> m;
        m.alloc(64);
        fill(m.get(), 64, 3);
        unsigned char* p = m.get();
        dev.fail_at = dev.attempts + 1;
        kv("r", m.fit_keep(128, 256, 40, copy_ok)); kv("same_ptr", m.get() == p); kv("bytes", (long long)m.bytes());
        kv("contents_same", same(m.get(), 64, 3)); kv("frees_inside", dev.frees);
    }
    counters();

    scenario("move_construct");
    {
        DevMem<char> a;
        a.alloc(100);
        char* p = a.get();
        DevMem<char> b(std::move(a));
        kv("source_empty", a.get() == nullptr && a.bytes() == 0); kv("target_has", b.get() == p && b.bytes() == 100);
        kv("frees_inside", dev.frees); kv("allocs_inside", dev.allocs);
    }
    counters();

    scenario("move_assign_into_empty");
    {
        DevMem<char> a, b;
        a.alloc(100);
        char* p = a.get();
        b = std::move(a);
        kv("source_empty", a.get() == nullptr && a.bytes() == 0); kv("target_has", b.get() == p && b.bytes() == 100);
        kv("frees_inside", dev.frees);
    }
    counters();

    scenario("move_assign_over_full");
    {
        DevMem<char> a, b;
        a.alloc(100); b.alloc(50);
        char* p = a.get();
        const int target_old = id_of(b.get());
        b = std::move(a);
        kv("source_empty", a.get() == nullptr && a.bytes() == 0); kv("target_has", b.get() == p && b.bytes() == 100);
        kv("old_freed", freed(target_old)); kv("frees_inside", dev.frees); kv("live_inside", (long long)dev.live);
    }
    counters();

    scenario("struct_assigned_from_empty");          // L = Lane{}
    {
        Several s;
        s.tag = 4; s.v.assign(3, 1);
        s.a.alloc(10); s.b.alloc(20); s.c.alloc(40);
        const int ia = id_of(s.a.get()), ib = id_of(s.b.get()), ic = id_of(s.c.get());
        s = Several{};
        kv("each_freed_once", freed(ia) == 1 && freed(ib) == 1 && freed(ic) == 1); kv("frees_inside", dev.frees);
        kv("members_empty", !s.a && !s.b && !s.c && s.a.bytes() + s.b.bytes() + s.c.bytes() == 0 && s.tag == 0 && s.v.empty());
        kv("live_inside", (long long)dev.live);
        s.b.alloc(8);          // and the struct is usable again
        Several t(std::move(s));
        kv("moved_whole", !s.b && t.b.bytes() == 8);
    }
    counters();

    scenario("pinned");
    {
        PinMem<unsigned> h;
        kv("r", h.alloc(256)); kv("bytes", (long long)h.bytes()); kv("pin_live_inside", (long long)pin.live);
        h.get()[63] = 1;
        dev.fail_at = 0; pin.fail_at = pin.attempts + 1;
        PinMem<unsigned> g;
        kv("r_fail", g.alloc(16)); kv("fail_null", g.get() == nullptr && g.bytes() == 0);
    }
    counters();
    return 0;
}
