// Communication between the ranks of a fit: the two lanes' all-reduces (RCCL, or the shared-memory test transport), the
// host exchange of the H-step round sums, and the vlgp_comm_* entry points.  The transport settings are
// read from the environment here, at set-up, and nowhere else.
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "ctx.h"
#include "host_exchange.h"

// ---- RCCL (loaded lazily: single-GPU use never touches it) ---------------
typedef struct { char internal[128]; } rccl_uid;
static struct {
    void* lib = nullptr;
    int (*get_uid)(rccl_uid*) = nullptr;
    int (*init_rank)(void**, int, rccl_uid, int) = nullptr;
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*destroy)(void*) = nullptr;
    const char* (*errstr)(int) = nullptr;
    int (*count)(void*, int*) = nullptr;  // ncclCommCount: what RCCL itself says the communicator spans
} g_rccl;

static int rccl_load(vlgp_ctx* ctx) {
    if (g_rccl.lib) return VLGP_OK;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return vlgp_fail(ctx, VLGP_ERR_COMM, "cannot load librccl.so: %s", dlerror());
    g_rccl.get_uid = (decltype(g_rccl.get_uid))dlsym(lib, "ncclGetUniqueId");
    g_rccl.init_rank = (decltype(g_rccl.init_rank))dlsym(lib, "ncclCommInitRank");
    g_rccl.all_reduce = (decltype(g_rccl.all_reduce))dlsym(lib, "ncclAllReduce");
    g_rccl.destroy = (decltype(g_rccl.destroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.errstr = (decltype(g_rccl.errstr))dlsym(lib, "ncclGetErrorString");
    g_rccl.count = (decltype(g_rccl.count))dlsym(lib, "ncclCommCount");
    if (!g_rccl.get_uid || !g_rccl.init_rank || !g_rccl.all_reduce || !g_rccl.destroy)
        return vlgp_fail(ctx, VLGP_ERR_COMM, "librccl.so lacks an expected symbol");
    g_rccl.lib = lib;
    return VLGP_OK;
}
static int rccl_fail(vlgp_ctx* ctx, const char* call, int lane, int rc) {
    return vlgp_fail(ctx, VLGP_ERR_COMM, "%s%s failed: %s", call, lane == LANE_M ? " (M-step lane)" : "",
                     g_rccl.errstr ? g_rccl.errstr(rc) : "?");
}

// ---- the two users of host_exchange.h -----------------------------------------------
// Shared-memory test transport: VLGP_COMM_TRANSPORT=shm replaces RCCL by an all-reduce through the host (device ->
// my slot, sum in rank order, host -> device).  It exists so that the full multi-rank protocol -- sharding, the
// per-Newton-iteration M-step reductions, the H-step rounds, the norms -- can be exercised by several processes that
// share ONE GPU (RCCL refuses two ranks on a device).  It is a test vehicle, not a data path: it sleeps between polls.
// Host exchange of the H-step round sums: with several ranks every round needs sum_ranks (ll, dll) for a handful of
// evaluations.  Each rank already has its own sums on the host (the round kernel's mailbox), so they are added there,
// busy-polled: ~3 us instead of an RCCL all-reduce plus a device-to-host copy (~50 us) on the latency-critical path
// of ~40 dependent rounds per EM iteration.  Single node only -- as is the rendezvous of the RCCL ids.
#define SHM_SLOT_DOUBLES (1 << 17)
#define HX_MAX_VALS 64
static bool shm_mode() {
    const char* t = getenv("VLGP_COMM_TRANSPORT");
    return t && strcmp(t, "shm") == 0;
}
// what a failed round says: the length did not fit a slot (the caller's error class), or a rank went silent
static int round_failed(vlgp_ctx* ctx, const char* who, int size_code, const HostExchange* c, long long n, int rc) {
    if (rc == HX_ERR_SIZE) return vlgp_fail(ctx, size_code, "%s: %lld doubles do not fit a slot of %d", who, n, c->cap);
    return vlgp_fail(ctx, VLGP_ERR_COMM, "%s: rank %d is not responding", who, c->silent);
}
static int shm_allreduce(vlgp_ctx* ctx, CommLane& L, double* d_buf, int64_t n) {
    double* mine = nullptr;
    int rc = hx_begin(L.shm, n, &mine);
    if (rc != HX_OK) return round_failed(ctx, "shm transport", VLGP_ERR_COMM, L.shm, n, rc);
    HIPCHK(ctx, hipMemcpyAsync(mine, d_buf, sizeof(double) * n, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    std::vector<double> sum((size_t)n);
    if ((rc = hx_finish(L.shm, sum.data())) != HX_OK) return round_failed(ctx, "shm transport", VLGP_ERR_COMM, L.shm, n, rc);
    HIPCHK(ctx, hipMemcpyAsync(d_buf, sum.data(), sizeof(double) * n, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    return VLGP_OK;
}
int vlgp_hx_allreduce(vlgp_ctx* ctx, double* vals, int n) {
    if (!ctx->hx) return vlgp_fail(ctx, VLGP_ERR_STATE, "no host exchange segment");
    double* mine = nullptr;
    int rc = hx_begin(ctx->hx, n, &mine);
    if (rc == HX_OK) {
        for (int i = 0; i < n; ++i) mine[i] = vals[i];
        rc = hx_finish(ctx->hx, vals);
    }
    return rc == HX_OK ? VLGP_OK : round_failed(ctx, "host exchange", VLGP_ERR_ARG, ctx->hx, n, rc);
}

// ---- lanes ----------------------------------------------------------------------
int vlgp_allreduce(vlgp_ctx* ctx, int lane, double* d_buf, int64_t n) {
    CommLane& L = ctx->lanes[lane];
    if (L.shm) return shm_allreduce(ctx, L, d_buf, n);
    if (!L.rccl) {  // one rank: nothing to add -- but never an M-step lane left closed beside an open main lane
        if (lane == LANE_M && ctx->lanes[LANE_MAIN].open())
            return vlgp_fail(ctx, VLGP_ERR_STATE, "multi-rank M-step needs the second communicator (vlgp_comm_init_aux)");
        return VLGP_OK;
    }
    const int rc = g_rccl.all_reduce(d_buf, d_buf, (size_t)n, /*ncclDouble*/ 8, /*ncclSum*/ 0, L.rccl, L.stream);
    return rc != 0 ? rccl_fail(ctx, "ncclAllReduce", lane, rc) : VLGP_OK;
}

static void close_lane(CommLane& L) {
    hx_close(L.shm);
    if (L.rccl && g_rccl.destroy) g_rccl.destroy(L.rccl);
    L.shm = nullptr;
    L.rccl = nullptr;
}
static int open_lane(vlgp_ctx* ctx, int lane, const char id[VLGP_UNIQUE_ID_BYTES], int rank, int world) {
    CommLane& L = ctx->lanes[lane];
    close_lane(L);
    if (shm_mode()) {
        const char* tmo = getenv("VLGP_SHM_TIMEOUT_S");
        L.shm = hx_open("/vlgp_shm_", id, VLGP_UNIQUE_ID_BYTES, rank, world, SHM_SLOT_DOUBLES, HX_SLEEP, tmo ? atof(tmo) : 60.0);
        if (L.shm) return VLGP_OK;
        return vlgp_fail(ctx, VLGP_ERR_COMM, "cannot open the shared-memory test transport%s", lane == LANE_M ? " (aux)" : "");
    }
    CHK(rccl_load(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    rccl_uid u;
    memcpy(u.internal, id, VLGP_UNIQUE_ID_BYTES);
    const int rc = g_rccl.init_rank(&L.rccl, world, u, rank);
    return rc != 0 ? rccl_fail(ctx, "ncclCommInitRank", lane, rc) : VLGP_OK;
}

void vlgp_comm_close(vlgp_ctx* ctx) {
    hx_close(ctx->hx);
    ctx->hx = nullptr;
    close_lane(ctx->lanes[LANE_M]);
    close_lane(ctx->lanes[LANE_MAIN]);
}

// ---- entry points -----------------------------------------------------------------
extern "C" int vlgp_comm_unique_id(char id[VLGP_UNIQUE_ID_BYTES]) {
    if (shm_mode()) {  // any bytes unique to this call will do
        memset(id, 0, VLGP_UNIQUE_ID_BYTES);
        static int counter = 0;
        snprintf(id, VLGP_UNIQUE_ID_BYTES, "shm-%d-%d-%ld", (int)getpid(), counter++, (long)time(nullptr));
        return VLGP_OK;
    }
    CHK(rccl_load(nullptr));
    rccl_uid u;
    const int rc = g_rccl.get_uid(&u);
    if (rc != 0) return vlgp_fail(nullptr, VLGP_ERR_COMM, "ncclGetUniqueId failed (%d)", rc);
    memcpy(id, u.internal, VLGP_UNIQUE_ID_BYTES);
    return VLGP_OK;
}

extern "C" int vlgp_comm_init(vlgp_ctx* ctx, const char id[VLGP_UNIQUE_ID_BYTES], int rank, int world) {
    NEED_CTX(ctx);
    if (world < 1 || rank < 0 || rank >= world) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad rank/world %d/%d", rank, world);
    vlgp_comm_close(ctx);  // a second vlgp_comm_init (transport fallback) starts over
    ctx->rank = rank;
    ctx->world = world;
    for (auto& us : ctx->sets) us.rows_all_ranks = 0.0;  // row totals exchanged under another communicator are stale
    // a single rank needs no communicator; VLGP_FORCE_RCCL=1 builds one anyway so
    // that the RCCL plumbing can be exercised on a one-GPU box (tests)
    if (world == 1 && !getenv("VLGP_FORCE_RCCL")) return VLGP_OK;
    if (world > 1 && !getenv("VLGP_NO_HOST_EXCHANGE"))  // optional: without it the H-step rounds use the device all-reduce
        ctx->hx = hx_open("/vlgp_hx_", id, VLGP_UNIQUE_ID_BYTES, rank, world, HX_MAX_VALS, HX_SPIN, 120.0);
    return open_lane(ctx, LANE_MAIN, id, rank, world);
}

extern "C" int vlgp_comm_init_aux(vlgp_ctx* ctx, const char id[VLGP_UNIQUE_ID_BYTES]) {
    NEED_CTX(ctx);
    if (ctx->world == 1 && !getenv("VLGP_FORCE_RCCL")) return VLGP_OK;
    if (!ctx->lanes[LANE_MAIN].open()) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_comm_init must precede vlgp_comm_init_aux");
    return open_lane(ctx, LANE_M, id, ctx->rank, ctx->world);
}

extern "C" int vlgp_comm_host_exchange(vlgp_ctx* ctx) { return ctx && ctx->hx ? 1 : 0; }
extern "C" int vlgp_comm_transport(vlgp_ctx* ctx) {
    return !ctx ? 0 : (ctx->lanes[LANE_MAIN].rccl ? 1 : (ctx->lanes[LANE_MAIN].shm ? 2 : 0));
}

extern "C" int vlgp_comm_rccl_ranks(vlgp_ctx* ctx, int* main_lane, int* m_lane) {
    NEED_CTX(ctx);
    if (!main_lane || !m_lane) return vlgp_fail(ctx, VLGP_ERR_ARG, "null out");
    int* out[2] = {main_lane, m_lane};
    for (int lane = 0; lane < 2; ++lane) {
        *out[lane] = 0;
        if (ctx->lanes[lane].rccl && g_rccl.count && g_rccl.count(ctx->lanes[lane].rccl, out[lane]) != 0) *out[lane] = -1;
    }
    return VLGP_OK;
}

extern "C" int vlgp_comm_allreduce_host(vlgp_ctx* ctx, double* buf, int n) {
    NEED_CTX(ctx);
    if (n < 0 || (n > 0 && !buf)) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad allreduce arguments");
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (!ctx->lanes[LANE_MAIN].open()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return VLGP_OK;
    }
    const int m = n > 0 ? n : 1;
    CHK(vlgp_ensure_work(ctx, m + 8));
    CHK(vlgp_ensure_pinned(ctx, m + 8));
    if (n > 0) memcpy(ctx->h_pinned, buf, sizeof(double) * n);
    else ctx->h_pinned[0] = 0.0;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_work, ctx->h_pinned, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
    CHK(vlgp_allreduce(ctx, LANE_MAIN, ctx->d_work, m));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctx->d_work, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n > 0) memcpy(buf, ctx->h_pinned, sizeof(double) * n);
    return VLGP_OK;
}
