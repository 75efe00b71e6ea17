// Host driver of csrc/dev_mem.h (tests/test_dev_mem.py): stand-ins for the HIP calls the header names, malloc-backed so
// that the address sanitizer sees a double free or a leak, counting every call and failing the k-th allocation on request.
// Usage: dev_mem_driver CASE.  A case prints "ok" and returns 0, or says what it expected and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct FakeStream { int id; };
struct FakeEvent { int id; };
typedef FakeStream* hipStream_t;
typedef FakeEvent* hipEvent_t;

static int n_malloc, n_free, n_host_malloc, n_host_free, n_sync, n_event_destroy, n_stream_destroy;
static int n_failed, fail_at;  // the k-th allocation from now (device and host counted together) fails; 0: none
static size_t last_bytes;
static unsigned last_flags;

static bool alloc_fails() {
    if (fail_at <= 0 || --fail_at > 0) return false;
    ++n_failed;
    return true;
}
static hipError_t hipMalloc(void** p, size_t bytes) {
    ++n_malloc;
    last_bytes = bytes;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    return hipSuccess;
}
static hipError_t hipFree(void* p) { ++n_free; free(p); return hipSuccess; }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    ++n_host_malloc;
    last_bytes = bytes;
    last_flags = flags;
    if (alloc_fails()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    return hipSuccess;
}
static hipError_t hipHostFree(void* p) { ++n_host_free; free(p); return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t) { ++n_sync; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { ++n_event_destroy; delete e; return hipSuccess; }
static hipError_t hipStreamDestroy(hipStream_t s) { ++n_stream_destroy; delete s; return hipSuccess; }

#include "dev_mem.h"

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("%s:%d: expected %s\n", __FILE__, __LINE__, #cond);      \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int64_t live(int i) { return g_live_memory[i].load(); }
static bool all_zero() { return !live(0) && !live(1) && !live(2) && !live(3); }

static int freed_once_by_destruction() {
    {
        DevPtr<double> p;
        EXPECT(!p.owned() && !p.get());
        EXPECT(p.alloc(5) == hipSuccess && last_bytes == 40);
        EXPECT(p.owned() && p.get() && live(0) == 1 && live(1) == 40);
        p[4] = 1.0;  // (the implicit conversion: the block is 5 doubles)
    }
    EXPECT(n_malloc == 1 && n_free == 1);
    return 0;
}
static int freed_once_by_reset() {
    DevPtr<int> p;
    EXPECT(p.alloc(3) == hipSuccess && live(1) == 12);
    p.reset();
    EXPECT(n_free == 1 && !p.owned() && !p.get() && all_zero());
    p.reset();
    EXPECT(n_free == 1);
    return 0;
}
static int freed_once_by_second_alloc() {
    DevPtr<double> p;
    EXPECT(p.alloc(2) == hipSuccess);
    EXPECT(p.alloc(7) == hipSuccess);
    EXPECT(n_malloc == 2 && n_free == 1 && live(0) == 1 && live(1) == 56);
    p.reset();
    EXPECT(n_free == 2);
    return 0;
}
static int freed_once_by_move_assignment() {
    DevPtr<double> a, b;
    EXPECT(a.alloc(2) == hipSuccess && b.alloc(3) == hipSuccess);
    double* const pb = b.get();
    a = std::move(b);  // a's old block goes, b is empty
    EXPECT(n_free == 1 && a.get() == pb && a.owned() && !b.get() && !b.owned() && live(0) == 1 && live(1) == 24);
    a = std::move(a);  // (self-assignment keeps the block)
    EXPECT(n_free == 1 && a.get() == pb);
    a.reset();
    EXPECT(n_free == 2);
    return 0;
}
static int borrowed_never_freed() {
    double rows[4] = {};
    {
        DevPtr<double> p, q;
        p.borrow(rows);
        EXPECT(p.get() == rows && !p.owned() && all_zero());
        q = std::move(p);
        EXPECT(q.get() == rows && !q.owned() && !p.get());
        q.reset();
        EXPECT(!q.get());
        q.borrow(rows + 1);
        EXPECT(p.alloc(2) == hipSuccess);
        p.borrow(rows);  // an owned block goes when the owner borrows instead
        EXPECT(n_free == 1);
    }
    EXPECT(n_malloc == 1 && n_free == 1);
    return 0;
}
static int moved_from_is_empty() {
    DevPtr<double> a;
    EXPECT(a.alloc(2) == hipSuccess);
    double* const pa = a.get();
    DevPtr<double> b(std::move(a));
    EXPECT(!a.get() && !a.owned() && b.get() == pa && b.owned() && live(0) == 1);
    GrowBuf<double> g;
    EXPECT(g.ensure(3, 4) == hipSuccess);
    GrowBuf<double> h(std::move(g));
    EXPECT(g.len == 0 && !g.get() && h.len == 4 && h.get());
    g = std::move(h);
    EXPECT(h.len == 0 && !h.get() && g.len == 4 && n_free == 0);
    return 0;
}
static int failed_alloc_leaves_empty() {
    DevPtr<double> p;
    EXPECT(p.alloc(2) == hipSuccess);
    fail_at = 1;
    EXPECT(p.alloc(9) != hipSuccess);
    EXPECT(!p.get() && !p.owned() && n_free == 1 && all_zero());
    HostPtr<double> h;
    fail_at = 1;
    EXPECT(h.alloc(9, 1) != hipSuccess && !h.get() && all_zero());
    return 0;
}
static int ensure_within_len_makes_no_call() {
    GrowBuf<double> g;
    FakeStream st{1};
    EXPECT(g.ensure(10, 12, &st) == hipSuccess);
    const int m = n_malloc, f = n_free, s = n_sync;
    double* const p = g.get();
    EXPECT(g.ensure(12, 99, &st) == hipSuccess && g.ensure(0, 99, &st) == hipSuccess && g.ensure(1, 99) == hipSuccess);
    EXPECT(n_malloc == m && n_free == f && n_sync == s && g.get() == p && g.len == 12);
    return 0;
}
static int ensure_allocates_the_capacity() {
    GrowBuf<double> g;
    EXPECT(g.ensure(10, 10 + 10 / 4 + 1024) == hipSuccess);
    EXPECT(last_bytes == 8 * 1036 && g.len == 1036 && live(0) == 1 && live(1) == 8 * 1036);
    EXPECT(g.ensure(1037, 1037) == hipSuccess);  // exact size
    EXPECT(last_bytes == 8 * 1037 && g.len == 1037 && n_malloc == 2 && n_free == 1 && live(1) == 8 * 1037);
    HostGrowBuf<double> h;
    EXPECT(h.ensure(5, 5 + 1024, nullptr, 3) == hipSuccess);
    EXPECT(n_host_malloc == 1 && last_flags == 3 && last_bytes == 8 * 1029 && live(2) == 1 && live(3) == 8 * 1029);
    return 0;
}
static int ensure_synchronises_with_a_stream_only() {
    GrowBuf<double> g;
    FakeStream st{1};
    EXPECT(g.ensure(4, 4) == hipSuccess && n_sync == 0);
    EXPECT(g.ensure(8, 8, &st) == hipSuccess && n_sync == 1);
    EXPECT(g.ensure(9, 9, nullptr) == hipSuccess && n_sync == 1);
    return 0;
}
static int failed_growth_leaves_empty() {
    GrowBuf<double> g;
    EXPECT(g.ensure(4, 4) == hipSuccess);
    fail_at = 1;
    EXPECT(g.ensure(8, 8) != hipSuccess);
    EXPECT(!g.get() && g.len == 0 && n_free == 1 && all_zero());  // not: the old length at address zero
    EXPECT(g.ensure(2, 2) == hipSuccess && g.len == 2 && g.get());  // the next call allocates again
    return 0;
}
static int host_blocks_and_handles() {
    {
        HostPtr<double> h;
        EXPECT(h.alloc(8, 2) == hipSuccess && last_flags == 2 && live(2) == 1 && live(3) == 64 && live(0) == 0);
        DevPtr<double> view;
        view.borrow(h.get());
        DevEvent e, e2;
        DevStream s;
        EXPECT(!e && !s);
        *e.put() = new FakeEvent{1};
        *s.put() = new FakeStream{2};
        EXPECT(e.get() && s.get());
        e2 = std::move(e);
        EXPECT(!e.get() && e2.get() && n_event_destroy == 0);
        *e2.put() = new FakeEvent{3};  // creating again destroys the one held
        EXPECT(n_event_destroy == 1);
    }
    EXPECT(n_host_malloc == 1 && n_host_free == 1 && n_free == 0 && n_event_destroy == 2 && n_stream_destroy == 1);
    return 0;
}

int main(int argc, char** argv) {
    struct Case { const char* name; int (*run)(); };
    const Case cases[] = {
        {"freed_once_by_destruction", freed_once_by_destruction},
        {"freed_once_by_reset", freed_once_by_reset},
        {"freed_once_by_second_alloc", freed_once_by_second_alloc},
        {"freed_once_by_move_assignment", freed_once_by_move_assignment},
        {"borrowed_never_freed", borrowed_never_freed},
        {"moved_from_is_empty", moved_from_is_empty},
        {"failed_alloc_leaves_empty", failed_alloc_leaves_empty},
        {"ensure_within_len_makes_no_call", ensure_within_len_makes_no_call},
        {"ensure_allocates_the_capacity", ensure_allocates_the_capacity},
        {"ensure_synchronises_with_a_stream_only", ensure_synchronises_with_a_stream_only},
        {"failed_growth_leaves_empty", failed_growth_leaves_empty},
        {"host_blocks_and_handles", host_blocks_and_handles},
    };
    if (argc == 2 && !strcmp(argv[1], "list")) {
        for (const Case& c : cases) printf("%s\n", c.name);
        return 0;
    }
    for (const Case& c : cases) {
        if (argc != 2 || strcmp(argv[1], c.name)) continue;
        if (c.run()) return 1;
        // every owner of the case is gone: one free per block handed out, the four counters back at zero
        if (n_malloc + n_host_malloc - n_failed != n_free + n_host_free || !all_zero()) {
            printf("%s: %d + %d allocations (%d failed), %d + %d frees, live %lld %lld %lld %lld\n", c.name, n_malloc, n_host_malloc,
                   n_failed, n_free, n_host_free, (long long)live(0), (long long)live(1), (long long)live(2), (long long)live(3));
            return 1;
        }
        printf("ok\n");
        return 0;
    }
    printf("usage: dev_mem_driver list | CASE\n");
    return 2;
}
