// Sum of doubles over the ranks of ONE node through a POSIX shared-memory segment, in rank order starting from 0.0:
// every rank gets the same bits.  libc / POSIX / <chrono> only (no HIP), so the protocol is tested without a GPU
// (tests/host_exchange_driver.cpp).  Two users (comm.hip): the shared-memory test transport and the H-step round sums.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <sys/mman.h>
#include <unistd.h>

#include <chrono>

#define HX_MAX_RANKS 16
enum { HX_OK = 0, HX_ERR_SIZE = 1, HX_ERR_RANK = 2 };  // HX_ERR_RANK: rank HostExchange::silent did not answer in time
// How a rank waits for the others: HX_SLEEP polls every 20 us and looks at the clock each time; HX_SPIN busy-polls and
// looks at the clock every 65 536 spins only (the H-step exchange: ~40 dependent rounds per EM iteration wait on it).
enum HxWait { HX_SLEEP, HX_SPIN };

// The segment: per rank a `ready` and a `done` round counter, one cache line each, then per rank a slot of `cap`
// doubles.  No ABI (every rank runs the same library); a fresh segment is zero-filled, the first round is number 1.
struct HostExchange {
    char* base = nullptr;
    size_t bytes = 0;
    int rank = 0, world = 1, cap = 0;
    HxWait wait = HX_SLEEP;
    double timeout_s = 60.0;  // a rank that died must not hang the others: every wait gives up after this long
    long long seq = 0;        // the round this rank is in
    int64_t n = 0;            // ... and its length (hx_begin)
    int silent = -1;
    char name[64];
    long long* ready(int k) const { return reinterpret_cast<long long*>(base) + 8 * k; }
    long long* done(int k) const { return ready(HX_MAX_RANKS + k); }
    double* slot(int k) const { return reinterpret_cast<double*>(ready(2 * HX_MAX_RANKS)) + (size_t)cap * k; }
};

// Every rank opens the segment named by (prefix, id) and maps it; null when that fails or world > HX_MAX_RANKS.
inline HostExchange* hx_open(const char* prefix, const char* id, int id_bytes, int rank, int world, int cap, HxWait wait,
                             double timeout_s) {
    if (world < 1 || world > HX_MAX_RANKS || rank < 0 || rank >= world || cap < 1) return nullptr;
    HostExchange* c = new HostExchange();
    c->rank = rank; c->world = world; c->cap = cap; c->wait = wait; c->timeout_s = timeout_s;
    c->bytes = 2 * HX_MAX_RANKS * 64 + sizeof(double) * HX_MAX_RANKS * (size_t)cap;
    unsigned long long h = 1469598103934665603ULL;  // FNV-1a of the id
    for (int i = 0; i < id_bytes; ++i) h = (h ^ (unsigned char)id[i]) * 1099511628211ULL;
    snprintf(c->name, sizeof(c->name), "%s%016llx", prefix, h);
    const int fd = shm_open(c->name, O_CREAT | O_RDWR, 0600);
    void* p = MAP_FAILED;
    if (fd >= 0 && ftruncate(fd, (off_t)c->bytes) == 0) p = mmap(nullptr, c->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (fd >= 0) close(fd);
    if (p == MAP_FAILED) { delete c; return nullptr; }
    c->base = static_cast<char*>(p);
    return c;
}

inline void hx_close(HostExchange* c) {  // rank 0 removes the name
    if (!c) return;
    munmap(c->base, c->bytes);
    if (c->rank == 0) shm_unlink(c->name);
    delete c;
}

// every rank's `done` (or `ready`) counter has reached `want`, or HX_ERR_RANK with the first rank that has not in c->silent
inline int hx_wait_all(HostExchange* c, bool done, long long want) {
    for (int k = 0; k < c->world; ++k) {
        const long long* p = done ? c->done(k) : c->ready(k);
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 1; __atomic_load_n(p, __ATOMIC_ACQUIRE) < want; ++spins) {
            if (c->wait == HX_SLEEP) usleep(20);
            else if (spins & 0xffff) continue;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->timeout_s) {
                c->silent = k;
                return HX_ERR_RANK;
            }
        }
    }
    return HX_OK;
}

// A round in two steps, so that the caller fills its slot however it likes.  hx_begin: wait until nobody still reads my
// slot from the previous round; *mine = my slot, room for n doubles.  n out of range: HX_ERR_SIZE, nothing touched.
inline int hx_begin(HostExchange* c, int64_t n, double** mine) {
    if (n < 0 || n > c->cap) return HX_ERR_SIZE;
    c->n = n;
    ++c->seq;
    const int rc = hx_wait_all(c, true, c->seq - 1);
    *mine = c->slot(c->rank);
    return rc;
}

// hx_finish: publish my slot, wait for every rank's, out[0 .. n) = 0.0 + slot 0 + slot 1 + ..., then release the slots.
inline int hx_finish(HostExchange* c, double* out) {
    __atomic_store_n(c->ready(c->rank), c->seq, __ATOMIC_RELEASE);
    const int rc = hx_wait_all(c, false, c->seq);
    if (rc != HX_OK) return rc;
    for (int64_t i = 0; i < c->n; ++i) out[i] = 0.0;
    for (int k = 0; k < c->world; ++k) {  // fixed rank order
        const double* s = c->slot(k);
        for (int64_t i = 0; i < c->n; ++i) out[i] += s[i];
    }
    __atomic_store_n(c->done(c->rank), c->seq, __ATOMIC_RELEASE);
    return HX_OK;
}
