// C ABI of libvlgp_hip.so (include/vlgp_hip.h): handle management, host<->device
// marshalling and the thin wrappers around the kernel launchers (communication between ranks: comm.hip; the read-only
// scores of a set: eval_api.hip).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include <algorithm>
#include <new>

#include "call_block.h"
#include "ctx.h"

static thread_local std::string g_create_err;

int vlgp_fail(vlgp_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_err = buf;
    return code;
}

static int dev_alloc(vlgp_ctx* ctx, DevPtr<double>& p, int64_t n, bool zero) {
    if (n <= 0) n = 1;
    HIPCHK(ctx, p.alloc((size_t)n));
    if (zero) HIPCHK(ctx, hipMemsetAsync(p, 0, (size_t)n * sizeof(double), ctx->stream));
    return VLGP_OK;
}

// a workspace of at least n doubles, grown with headroom once the stream that uses it has drained
int vlgp_ensure_work(vlgp_ctx* ctx, int64_t n) {
    HIPCHK(ctx, ctx->d_work.ensure(n, n + n / 4 + 1024, ctx->stream));
    return VLGP_OK;
}
int vlgp_ensure_work_m(vlgp_ctx* ctx, int64_t n) {
    HIPCHK(ctx, ctx->d_work_m.ensure(n, n + n / 4 + 1024, ctx->mstream));
    return VLGP_OK;
}

// wait for a queued norms pass (vlgp_norms_begin): its sequence word in mapped host memory
static int wait_norms(vlgp_ctx* ctx) {
    if (ctx->x_pending != 1) return VLGP_OK;
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(ctx->h_xres + 2);
    unsigned spins = 0;
    while (*flag != ctx->x_seq) {
        if ((++spins & 0xfff) == 0) {  // a faulted kernel must not hang the host
            const hipError_t qe = hipStreamQuery(ctx->stream);
            if (qe == hipSuccess) {
                if (*flag == ctx->x_seq) break;
                if ((spins >> 12) > 64) return vlgp_fail(ctx, VLGP_ERR_HIP, "norms kernel finished without publishing");
            } else if (qe != hipErrorNotReady) {
                return vlgp_fail(ctx, VLGP_ERR_HIP, "norms kernel failed: %s", hipGetErrorString(qe));
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return VLGP_OK;
}

int vlgp_join_m(vlgp_ctx* ctx) {
    ++ctx->write_epoch;  // the callers are the entry points that read or write parameters / unit state (vlgp_hstep_prepare)
    // a pending norms pass (vlgp_norms_begin) reads mu, v, dmu on its own stream: the same callers wait for it
    CHK(wait_norms(ctx));
    if (!ctx->m_pending) return VLGP_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_m_done));  // m_pending is cleared by vlgp_mstep_end
    return VLGP_OK;
}

int vlgp_ensure_pinned(vlgp_ctx* ctx, int64_t n) {
    HIPCHK(ctx, ctx->h_pinned.ensure(n, n + 1024, ctx->stream, hipHostMallocDefault));
    return VLGP_OK;
}

int vlgp_raise_lds(vlgp_ctx* ctx, const void* fn, int bytes) {
    if (std::find(ctx->lds_attr_done.begin(), ctx->lds_attr_done.end(), fn) != ctx->lds_attr_done.end()) return VLGP_OK;
    HIPCHK(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    ctx->lds_attr_done.push_back(fn);
    return VLGP_OK;
}

UnitSet* vlgp_get_set(vlgp_ctx* ctx, int set, bool must_be_valid) {
    if (set < 0 || set >= VLGP_MAX_SETS) {
        vlgp_fail(ctx, VLGP_ERR_ARG, "unit set index %d out of range [0, %d)", set, VLGP_MAX_SETS);
        return nullptr;
    }
    UnitSet* us = &ctx->sets[set];
    if (must_be_valid && !us->valid) {
        vlgp_fail(ctx, VLGP_ERR_STATE, "unit set %d is empty (upload or cut first)", set);
        return nullptr;
    }
    return us;
}

// ---- which entry point takes which kind of set -----------------------------------------------------
// ONE table: X(entry point, kinds it takes, what it says to a refused set that is not replicated).  A refused replicated
// set is told "<entry point> refuses a replicated set (...)"; the replicate calls say their text to every refused set.
// SET_FIT = not replicated, or a masked set of one replica: that one is the source's rows, units and y / x with its own
// mu, v, w, dmu and one mask bit per entry of y, so the entry points that read mu, v, w, dmu alone (norms, latent map,
// moments, H-step) take it as any set, update_w / update_v go through the split E-step's masked row passes and the
// M-step has masked kernels (mstep.hip).  Everything else would read a replicated set's aliased y / x with the replicas'
// row count, or mix the left-out channels and entries back in.  Without SET_SOURCE a set that is the source of replicas
// is refused as well: its rows must stay while replicas alias them.
#define NOT_REPLICATED (SET_PLAIN | SET_TILING | SET_COPIED | SET_SOURCE)
#define SET_ADMISSION(X)                                                                                              \
    X(vlgp_estep, SET_ANY, nullptr)                                                                                   \
    X(vlgp_download_units, SET_ANY, nullptr)                                                                          \
    X(vlgp_free_units, SET_ANY & ~SET_SOURCE, nullptr)                                                                \
    X(vlgp_upload_units, SET_ANY & ~SET_SOURCE, nullptr)                                                              \
    X(vlgp_loglik, SET_ANY & ~SET_COPIED, "vlgp_loglik on a copied cut: merge it and score the source set")           \
    X(vlgp_predictive, SET_ANY & ~SET_COPIED, "vlgp_predictive on a copied cut: merge it and score the source set")   \
    X(vlgp_calibration, SET_ANY & ~SET_COPIED, "vlgp_calibration on a copied cut: merge it and score the source set") \
    X(vlgp_predictive_cov, SET_ANY & ~SET_COPIED,                                                                     \
      "vlgp_predictive_cov on a copied cut: merge it and score the source set")                                       \
    X(vlgp_calibration_cov, SET_ANY & ~SET_COPIED,                                                                    \
      "vlgp_calibration_cov on a copied cut: merge it and score the source set")                                      \
    X(vlgp_pair_moments, SET_ANY & ~(SET_COPIED | SET_GROUPS),                                                        \
      "vlgp_pair_moments on a copied cut: merge it and score the source set")                                         \
    X(vlgp_pair_moments_cov, SET_ANY & ~(SET_COPIED | SET_GROUPS),                                                    \
      "vlgp_pair_moments_cov on a copied cut: merge it and score the source set")                                     \
    X(vlgp_lag_moments, SET_ANY & ~(SET_COPIED | SET_GROUPS),                                                         \
      "vlgp_lag_moments on a copied cut: merge it and score the source set")                                          \
    X(vlgp_update_w, SET_FIT | SET_SOURCE, nullptr)                                                                   \
    X(vlgp_update_v, SET_FIT | SET_SOURCE, nullptr)                                                                   \
    X(vlgp_mstep_begin, SET_FIT | SET_SOURCE, nullptr)                                                                \
    X(vlgp_hstep_objective, SET_FIT | SET_SOURCE, nullptr)                                                            \
    X(vlgp_hstep_prepare, SET_FIT | SET_SOURCE, nullptr)                                                              \
    X(vlgp_hstep_begin, SET_FIT | SET_SOURCE, nullptr)                                                                \
    X(vlgp_apply_latent_map, SET_FIT | SET_SOURCE, nullptr)                                                           \
    X(vlgp_norms, SET_FIT | SET_SOURCE, nullptr)                                                                      \
    X(vlgp_norms_begin, SET_FIT | SET_SOURCE, nullptr)                                                                \
    X(vlgp_latent_moments, SET_FIT | SET_SOURCE, nullptr)                                                             \
    X(vlgp_elbo, NOT_REPLICATED, nullptr)                                                                             \
    X(vlgp_forecast, NOT_REPLICATED, nullptr) /* (a cut is refused once its priors are bound: see there) */           \
    X(vlgp_marginal, NOT_REPLICATED, nullptr)                                                                         \
    X(vlgp_joint_laplace, NOT_REPLICATED, nullptr)                                                                    \
    X(vlgp_joint_posterior, NOT_REPLICATED | SET_MASKED_FIT, nullptr)                                                 \
    X(vlgp_joint_posterior_moments, NOT_REPLICATED | SET_MASKED_FIT, nullptr)                                         \
    X(vlgp_mstep_cov, NOT_REPLICATED, nullptr)                                                                        \
    X(vlgp_mstep_cov_masked, SET_MASKED_FIT,                                                                          \
      "vlgp_mstep_cov_masked takes a masked fit set (set %d has no mask: vlgp_mstep_cov takes it)")                   \
    X(vlgp_stash_mu, NOT_REPLICATED, nullptr)                                                                         \
    X(vlgp_set_overlaps, NOT_REPLICATED, nullptr) /* (and equal-length units that are no tiling cut: see there) */    \
    X(vlgp_unshare_mu, NOT_REPLICATED, nullptr)                                                                       \
    X(vlgp_project_units, NOT_REPLICATED, nullptr) /* (a tiling cut is refused after the arguments: see there) */     \
    X(vlgp_merge_units, SET_TILING | SET_COPIED | SET_SOURCE, "set %d is not a cut")                                  \
    X(vlgp_cut_units, SET_PLAIN | SET_COPIED | SET_SOURCE, "cannot cut a set that is itself a cut") /* the source */  \
    X(vlgp_replicate, SET_PLAIN | SET_SOURCE,                                                                         \
      "replicate a plain uploaded set (set %d is a cut, a replica or has overlaps)") /* the source, _groups / _masked */ \
    X(destination, SET_ANY & ~SET_SOURCE, nullptr) /* of vlgp_cut_units and the replicate calls: any set, or none yet */
#define X(name, kinds, refusal) \
    extern const Admission admit_##name; /* (ctx.h declares the ones eval_api.hip uses) */ \
    const Admission admit_##name = {#name, kinds, refusal};
SET_ADMISSION(X)
#undef X

int admit(vlgp_ctx* ctx, int set, const UnitSet* us, const Admission& a) {
    if (us->is_source() && !(a.kinds & SET_SOURCE))
        return vlgp_fail(ctx, VLGP_ERR_STATE, "set %d is the source of a replicated set: free the replicas first", set);
    if (us->is(a.kinds)) return VLGP_OK;
    if (us->is(SET_REPLICATED) && &a != &admit_vlgp_replicate)
        return vlgp_fail(ctx, VLGP_ERR_STATE, "%s refuses a replicated set (leave-one-out replicas of set %d: "
                         "E-step, download, loglik and free only)", a.what, us->rep.src);
    return vlgp_fail(ctx, VLGP_ERR_STATE, a.refusal, set);
}

// How a set-taking entry point opens (the OPEN_* flags: ctx.h), in this order, then the set and its admission.
#define NEED_PARAMS(ctx) \
    if (!(ctx)->have_params) return vlgp_fail(ctx, VLGP_ERR_STATE, "parameters not set (vlgp_set_params)")
int open_set(vlgp_ctx* ctx, int set, unsigned how, UnitSet** out, const Admission* a) {
    NEED_CTX(ctx);
    if (how & OPEN_COLLECT) CHK(vlgp_prior_collect(ctx));
    if (how & OPEN_STALE) ctx->hmom_us = nullptr;
    if (how & OPEN_JOIN) CHK(vlgp_join_m(ctx));
    if (how & OPEN_WAIT) {
        CHK(wait_norms(ctx));
        if (ctx->m_pending) HIPCHK(ctx, hipEventSynchronize(ctx->ev_m_done));
    }
    if (how & OPEN_PARAMS) NEED_PARAMS(ctx);
    if (how & OPEN_DEVICE) HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (!(*out = vlgp_get_set(ctx, set, !(how & OPEN_EMPTY)))) return VLGP_ERR_ARG;
    return a ? admit(ctx, set, *out, *a) : VLGP_OK;  // (null: the entry point checks its arguments first, then admits)
}
// ... and one that makes set dst out of set src (a cut, replicas): both slots, then the call's own arguments
static int open_pair(vlgp_ctx* ctx, int src, int dst, bool bad_args, const char* bad, UnitSet** s, UnitSet** d) {
    CHK(open_set(ctx, src, OPEN_STALE | OPEN_JOIN | OPEN_DEVICE, s, nullptr));
    if (!(*d = vlgp_get_set(ctx, dst, false))) return VLGP_ERR_ARG;
    return bad_args ? vlgp_fail(ctx, VLGP_ERR_ARG, "%s", bad) : VLGP_OK;
}

// ---- profiling -----------------------------------------------------------
void vlgp_prof_begin(vlgp_ctx* ctx, int kind, hipStream_t st) {
    if (!ctx->prof_on) return;
    DevEvent a, b;
    if (hipEventCreate(a.put()) != hipSuccess || hipEventCreate(b.put()) != hipSuccess) return;
    (void)hipEventRecord(a, st ? st : ctx->stream.get());
    ctx->pending.push_back({kind, std::move(a), std::move(b), 0.0, false});
}
void vlgp_prof_end(vlgp_ctx* ctx, int kind, double units, hipStream_t st) {
    if (!ctx->prof_on) return;
    // brackets nest (a whole E-step around the sampled launches inside it): close the innermost open one of this kind
    for (auto it = ctx->pending.rbegin(); it != ctx->pending.rend(); ++it) {
        if (it->kind != kind || it->done) continue;
        it->units = units;
        it->done = true;
        (void)hipEventRecord(it->b, st ? st : ctx->stream.get());
        return;
    }
}
static void prof_drain(vlgp_ctx* ctx) {
    if (ctx->pending.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->mstream);
    for (auto& p : ctx->pending) {
        float ms = 0.f;
        if (p.done && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            ctx->prof[p.kind].launches += 1;
            ctx->prof[p.kind].ms += ms;
            ctx->prof[p.kind].units += p.units;
        }
    }
    ctx->pending.clear();
}

// ---- lifetime --------------------------------------------------------------
extern "C" int vlgp_abi_version(void) { return VLGP_ABI_VERSION; }

extern "C" int vlgp_debug_live_memory(int64_t out[4]) {
    if (!out) return vlgp_fail(nullptr, VLGP_ERR_ARG, "null output");
    for (int i = 0; i < 4; ++i) out[i] = g_live_memory[i].load();
    return VLGP_OK;
}

extern "C" int vlgp_device_count(int* count) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return vlgp_fail(nullptr, VLGP_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return VLGP_OK;
}

extern "C" const char* vlgp_last_error(vlgp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// wait for the stream, give the source its user count back, release what the set owns (what it borrows stays: dev_mem.h)
static void free_set(vlgp_ctx* ctx, UnitSet& us) {
    if (!us.valid) return;
    (void)hipStreamSynchronize(ctx->stream);
    if (us.rep.src >= 0) ctx->sets[us.rep.src].rep_users--;
    us = UnitSet();
}

// A set is built in a local UnitSet and moved into its slot when every step has succeeded; a source counts its user then.
// A step that fails leaves the slot empty (its old contents went first) and the local releases what it had allocated.
static int commit_set(UnitSet& slot, UnitSet& built, UnitSet* source) {
    built.valid = true;
    slot = std::move(built);
    if (source) source->rep_users++;
    return VLGP_OK;
}

// ... and, first, the tiling cuts that share its rows
static void free_with_tiling_cuts(vlgp_ctx* ctx, int set) {
    for (auto& other : ctx->sets)
        if (other.valid && other.is(SET_TILING) && other.parent == set) free_set(ctx, other);
    free_set(ctx, ctx->sets[set]);
}

extern "C" int vlgp_create(int device, int N, int L, int P, int R, const uint8_t* gauss_mask, vlgp_ctx** out) {
    if (!out) return vlgp_fail(nullptr, VLGP_ERR_ARG, "null output handle");
    *out = nullptr;
    if (N < 1 || L < 1 || P < 1 || R < 1) return vlgp_fail(nullptr, VLGP_ERR_ARG, "N, L, P, R must be positive");
    if (R > VLGP_MAX_RANK) return vlgp_fail(nullptr, VLGP_ERR_ARG, "rank %d exceeds VLGP_MAX_RANK=%d", R, VLGP_MAX_RANK);
    if (L > VLGP_MAX_L) return vlgp_fail(nullptr, VLGP_ERR_ARG, "at most %d latents supported, got %d", VLGP_MAX_L, L);
    if (P > VLGP_MAX_XDIM) return vlgp_fail(nullptr, VLGP_ERR_ARG, "at most %d regressors supported, got %d", VLGP_MAX_XDIM, P);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return vlgp_fail(nullptr, VLGP_ERR_HIP, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return vlgp_fail(nullptr, VLGP_ERR_ARG, "device %d out of range (have %d)", device, ndev);
    vlgp_ctx* ctx = new (std::nothrow) vlgp_ctx();
    if (!ctx) return vlgp_fail(nullptr, VLGP_ERR_HIP, "out of host memory");
    ctx->dev = device; ctx->N = N; ctx->L = L; ctx->P = P; ctx->R = R;
    vlgp_read_switches(ctx);
#define CREATE_CHK(call)                                                                  \
    do {                                                                                  \
        hipError_t e2 = (call);                                                           \
        if (e2 != hipSuccess) {                                                           \
            vlgp_fail(nullptr, VLGP_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e2)); \
            delete ctx;                                                                   \
            return VLGP_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)
    CREATE_CHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    CREATE_CHK(hipGetDeviceProperties(&prop, device));
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (prop.sharedMemPerBlock > 0) ctx->lds_max = (int)prop.sharedMemPerBlock;
    {   // the main stream carries the latency-critical H-step rounds: give it the highest
        // priority, the M-step lane the lowest, so that M kernels only fill what H leaves idle
        int prio_lo = 0, prio_hi = 0;
        CREATE_CHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        CREATE_CHK(hipStreamCreateWithPriority(ctx->stream.put(), hipStreamNonBlocking, prio_hi));
        CREATE_CHK(hipStreamCreateWithPriority(ctx->mstream.put(), hipStreamNonBlocking, prio_lo));
        ctx->lanes[LANE_MAIN].stream = ctx->stream;
        ctx->lanes[LANE_M].stream = ctx->mstream;
    }
    CREATE_CHK(hipEventCreateWithFlags(ctx->ev_fork.put(), hipEventDisableTiming));
    CREATE_CHK(hipEventCreate(ctx->ev_m_start.put()));
    CREATE_CHK(hipEventCreate(ctx->ev_m_done.put()));
    CREATE_CHK(ctx->d_fail_m.alloc(1));
    CREATE_CHK(hipMemset(ctx->d_fail_m, 0, sizeof(int)));
    ctx->gauss.assign(N, 0);
    std::vector<int> gi(N, 0);
    for (int n = 0; n < N; ++n) {
        const uint8_t g = gauss_mask ? gauss_mask[n] : 0;
        ctx->gauss[n] = g ? 1 : 0;
        gi[n] = g ? 1 : 0;
        ctx->n_gauss += g ? 1 : 0;
    }
    CREATE_CHK(ctx->d_gauss.alloc(N));
    CREATE_CHK(hipMemcpy(ctx->d_gauss, gi.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    CREATE_CHK(ctx->d_a.alloc((size_t)L * N));
    CREATE_CHK(ctx->d_da.alloc((size_t)L * N));
    CREATE_CHK(ctx->d_b.alloc((size_t)P * N));
    CREATE_CHK(ctx->d_db.alloc((size_t)P * N));
    CREATE_CHK(ctx->d_noise.alloc(N));
    CREATE_CHK(hipMemset(ctx->d_da, 0, sizeof(double) * L * N));
    CREATE_CHK(hipMemset(ctx->d_db, 0, sizeof(double) * P * N));
    CREATE_CHK(ctx->d_fail.alloc(1));
    CREATE_CHK(hipMemset(ctx->d_fail, 0, sizeof(int)));
#undef CREATE_CHK
    *out = ctx;
    return VLGP_OK;
}

static void free_priors(vlgp_ctx* ctx) {
    ctx->prior_pending.clear();  // (every caller has synchronised the stream; the ranks go with the priors)
    ctx->priors.clear();
}

extern "C" int vlgp_destroy(vlgp_ctx* ctx) {
    if (!ctx) return VLGP_OK;
    (void)hipSetDevice(ctx->dev);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->mstream) (void)hipStreamSynchronize(ctx->mstream);
    if (ctx->m_graph_exec) (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(ctx->m_graph_exec));
    ctx->m_graph_exec = nullptr;
    ctx->m_pending = false;
    prof_drain(ctx);
    vlgp_comm_close(ctx);
    // aliased sets first, then owners
    for (int pass = 0; pass < 2; ++pass)
        for (auto& us : ctx->sets)
            if (us.valid && (pass == 1 || us.is(SET_TILING))) free_set(ctx, us);
    delete ctx;  // every buffer, event and stream is a member that releases itself (dev_mem.h)
    return VLGP_OK;
}

extern "C" int vlgp_synchronize(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    CHK(vlgp_join_m(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_synchronize_main(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_estep_wait(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    if (ctx->e_done_valid) HIPCHK(ctx, hipEventSynchronize(ctx->ev_e_done));
    else HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

// ---- unit sets -------------------------------------------------------------
static int set_offsets(vlgp_ctx* ctx, UnitSet& us, int M, const int64_t* off) {
    us.M = M;
    us.off.assign(off, off + M + 1);
    us.rows = off[M] - off[0];
    us.Tmax = 0;
    us.Tmin = 0x7fffffff;
    for (int m = 0; m < M; ++m) {
        const int64_t T = off[m + 1] - off[m];
        if (T < 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "unit %d has %lld rows", m, (long long)T);
        us.Tmax = std::max<int>(us.Tmax, (int)T);
        us.Tmin = std::min<int>(us.Tmin, (int)T);
    }
    HIPCHK(ctx, us.d_off.alloc((size_t)M + 1));
    HIPCHK(ctx, hipMemcpyAsync(us.d_off, us.off.data(), sizeof(int64_t) * (M + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, us.d_unit_prior.alloc(M));
    us.prior_epoch = 0;
    return VLGP_OK;
}

static int up(vlgp_ctx* ctx, DevPtr<double>& dst, const double* src, int64_t n) {
    CHK(dev_alloc(ctx, dst, n, src == nullptr));
    if (src) HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_upload_units(vlgp_ctx* ctx, int set, int M, const int64_t* offsets, const double* y,
                                 const double* x, const double* mu, const double* v, const double* w) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_STALE | OPEN_JOIN | OPEN_DEVICE | OPEN_EMPTY, &us, &admit_vlgp_upload_units));
    if (M < 1 || !offsets || !y) return vlgp_fail(ctx, VLGP_ERR_ARG, "upload needs M >= 1, offsets and y");
    if (offsets[0] != 0) return vlgp_fail(ctx, VLGP_ERR_ARG, "offsets[0] must be 0");
    if (!x && ctx->P != 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "x == NULL (all ones) requires xdim == 1");
    free_with_tiling_cuts(ctx, set);
    UnitSet made;
    CHK(set_offsets(ctx, made, M, offsets));
    const int64_t rows = made.rows;
    CHK(up(ctx, made.y, y, rows * ctx->N));
    made.x_ones = (x == nullptr);
    if (x) CHK(up(ctx, made.x, x, rows * ctx->P * ctx->N));
    CHK(up(ctx, made.mu, mu, rows * ctx->L));
    CHK(up(ctx, made.v, v, rows * ctx->L));
    CHK(up(ctx, made.w, w, rows * ctx->L));
    CHK(dev_alloc(ctx, made.dmu, rows * ctx->L, true));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // host buffers are the caller's again
    return commit_set(*us, made, nullptr);
}

extern "C" int vlgp_cut_units(vlgp_ctx* ctx, int src, int dst, int M_dst, const int64_t* start, int window) {
    UnitSet *s = nullptr, *d = nullptr;
    CHK(open_pair(ctx, src, dst, src == dst || M_dst < 1 || window < 1 || !start, "bad cut arguments", &s, &d));
    CHK(admit(ctx, src, s, admit_vlgp_cut_units));
    CHK(admit(ctx, dst, d, admit_destination));
    bool exact = (int64_t)M_dst * window == s->rows;
    for (int k = 0; k < M_dst; ++k) {
        if (start[k] < 0 || start[k] + window > s->rows)
            return vlgp_fail(ctx, VLGP_ERR_ARG, "segment %d [%lld, +%d) outside the source set", k, (long long)start[k], window);
        if (start[k] != (int64_t)k * window) exact = false;
    }
    free_set(ctx, *d);
    UnitSet made;
    std::vector<int64_t> off(M_dst + 1);
    for (int k = 0; k <= M_dst; ++k) off[k] = (int64_t)k * window;
    CHK(set_offsets(ctx, made, M_dst, off.data()));
    made.parent = src;
    made.x_ones = s->x_ones;
    made.src_start.assign(start, start + M_dst);
    HIPCHK(ctx, made.d_src_start.alloc(M_dst));
    HIPCHK(ctx, hipMemcpyAsync(made.d_src_start, start, sizeof(int64_t) * M_dst, hipMemcpyHostToDevice, ctx->stream));
    const int64_t rows = made.rows;
    CHK(dev_alloc(ctx, made.dmu, rows * ctx->L, true));
    made.alias = exact;
    if (exact) {  // a tiling cut: the parent's rows
        made.y.borrow(s->y); made.x.borrow(s->x); made.mu.borrow(s->mu); made.v.borrow(s->v); made.w.borrow(s->w);
    } else {
        CHK(dev_alloc(ctx, made.y, rows * ctx->N, false));
        if (!s->x_ones) CHK(dev_alloc(ctx, made.x, rows * ctx->P * ctx->N, false));
        CHK(dev_alloc(ctx, made.mu, rows * ctx->L, false));
        CHK(dev_alloc(ctx, made.v, rows * ctx->L, false));
        CHK(dev_alloc(ctx, made.w, rows * ctx->L, false));
        CHK(launch_gather(ctx, *s, made, window));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return commit_set(*d, made, nullptr);
}

extern "C" int vlgp_merge_units(vlgp_ctx* ctx, int cut_set) {
    UnitSet* c = nullptr;
    CHK(open_set(ctx, cut_set, OPEN_STALE | OPEN_JOIN, &c, &admit_vlgp_merge_units));
    if (c->is(SET_TILING)) return VLGP_OK;
    UnitSet* p = vlgp_get_set(ctx, c->parent, true);
    if (!p) return VLGP_ERR_STATE;
    return launch_scatter(ctx, *c, *p, (int)(c->off[1] - c->off[0]));
}

extern "C" int vlgp_stash_mu(vlgp_ctx* ctx, int set, int restore) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_JOIN, &us, &admit_vlgp_stash_mu));
    const size_t nb = (size_t)us->rows * ctx->L * sizeof(double);
    if (!restore) {
        if (!us->d_mu_stash) HIPCHK(ctx, us->d_mu_stash.alloc((size_t)us->rows * ctx->L));
        HIPCHK(ctx, hipMemcpyAsync(us->d_mu_stash, us->mu, nb, hipMemcpyDeviceToDevice, ctx->stream));
        return VLGP_OK;
    }
    if (!us->d_mu_stash) return vlgp_fail(ctx, VLGP_ERR_STATE, "set %d has no stashed mu", set);
    ctx->hmom_us = nullptr;
    HIPCHK(ctx, hipMemcpyAsync(us->mu, us->d_mu_stash, nb, hipMemcpyDeviceToDevice, ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_download_units(vlgp_ctx* ctx, int set, double* mu, double* v, double* w, double* dmu) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_JOIN, &us, &admit_vlgp_download_units));
    const size_t nb = (size_t)us->rows * ctx->L * sizeof(double);
    if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, us->mu, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (v) HIPCHK(ctx, hipMemcpyAsync(v, us->v, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (w) HIPCHK(ctx, hipMemcpyAsync(w, us->w, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (dmu) HIPCHK(ctx, hipMemcpyAsync(dmu, us->dmu, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_free_units(vlgp_ctx* ctx, int set) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_STALE | OPEN_JOIN | OPEN_EMPTY, &us, &admit_vlgp_free_units));
    free_with_tiling_cuts(ctx, set);
    return VLGP_OK;
}

// ---- leave-group-out replicas (their scores and every other read-only score: eval_api.hip) ----
// what every replicate call checks of its two sets once its own arguments are sound
static int replicas_check(vlgp_ctx* ctx, int src, int dst, int n_rep, const UnitSet* s, const UnitSet* d) {
    CHK(admit(ctx, src, s, admit_vlgp_replicate));
    if (!s->stage_start.empty()) return vlgp_fail(ctx, VLGP_ERR_STATE, admit_vlgp_replicate.refusal, src);
    CHK(admit(ctx, dst, d, admit_destination));
    if ((int64_t)n_rep * s->M > 0x7fffffffLL) return vlgp_fail(ctx, VLGP_ERR_ARG, "too many replicated units");
    return VLGP_OK;
}

// d := n_rep replicas of src, replica-major: offsets, y and x borrowed, mu, v, w, dmu its own, copies of the source's
// (enqueued; the caller adds its tables, synchronises and commits d to slot dst, whose old contents go here).
static int replicas_make(vlgp_ctx* ctx, int src, int dst, int n_rep, UnitSet* s, UnitSet* d) {
    free_with_tiling_cuts(ctx, dst);
    const int Ms = s->M, L = ctx->L;
    const int64_t rs = s->rows;
    std::vector<int64_t> off((size_t)n_rep * Ms + 1);
    for (int k = 0; k < n_rep; ++k)
        for (int m = 0; m < Ms; ++m) off[(size_t)k * Ms + m] = k * rs + s->off[m];
    off[(size_t)n_rep * Ms] = n_rep * rs;
    CHK(set_offsets(ctx, *d, n_rep * Ms, off.data()));
    d->rep.src = src;
    d->rep.n = n_rep;
    d->rep.rows_src = rs;
    d->rep.nw = (ctx->N + 63) / 64;
    d->x_ones = s->x_ones;
    d->y.borrow(s->y);  // a copy per replica would be rows x N doubles each
    d->x.borrow(s->x);
    const size_t nb = (size_t)rs * L * sizeof(double);
    CHK(dev_alloc(ctx, d->mu, n_rep * rs * L, false));
    CHK(dev_alloc(ctx, d->v, n_rep * rs * L, false));
    CHK(dev_alloc(ctx, d->w, n_rep * rs * L, false));
    CHK(dev_alloc(ctx, d->dmu, n_rep * rs * L, false));
    HIPCHK(ctx, d->rep.d_xa.alloc(sizeof(d->rep.xh) / sizeof(double)));
    for (int k = 0; k < n_rep; ++k) {
        const int64_t o = k * rs * L;
        HIPCHK(ctx, hipMemcpyAsync(d->mu + o, s->mu, nb, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d->v + o, s->v, nb, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d->w + o, s->w, nb, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d->dmu + o, s->dmu, nb, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return VLGP_OK;
}

extern "C" int vlgp_replicate_groups(vlgp_ctx* ctx, int src, int dst, int n_rep, const int* group_start,
                                     const int* channel) {
    UnitSet *s = nullptr, *d = nullptr;
    CHK(open_pair(ctx, src, dst, src == dst || n_rep < 1 || !channel || !group_start || group_start[0] != 0,
                  "bad replicate arguments", &s, &d));
    // the groups as bit masks (one bit per channel), the pairs' replicas: every argument is checked before any state moves
    const int nw = (ctx->N + 63) / 64;
    std::vector<unsigned long long> mask((size_t)n_rep * nw, 0ull);
    std::vector<int> pair_rep;
    for (int k = 0; k < n_rep; ++k) {
        if (group_start[k + 1] <= group_start[k])
            return vlgp_fail(ctx, VLGP_ERR_ARG, "replica %d leaves out an empty group of channels", k);
        for (int p = group_start[k]; p < group_start[k + 1]; ++p) {
            const int n = channel[p];
            if (n < 0 || n >= ctx->N)
                return vlgp_fail(ctx, VLGP_ERR_ARG, "replica %d leaves out channel %d, outside [0, %d)", k, n, ctx->N);
            unsigned long long& wd = mask[(size_t)k * nw + (n >> 6)];
            if ((wd >> (n & 63)) & 1ull)
                return vlgp_fail(ctx, VLGP_ERR_ARG, "replica %d leaves out channel %d twice", k, n);
            wd |= 1ull << (n & 63);
            pair_rep.push_back(k);
        }
    }
    const int n_pairs = group_start[n_rep];
    CHK(replicas_check(ctx, src, dst, n_rep, s, d));
    UnitSet made;
    CHK(replicas_make(ctx, src, dst, n_rep, s, &made));
    Replicas& r = made.rep;
    r.n_pairs = n_pairs;
    HIPCHK(ctx, r.d_ch.alloc(n_pairs));
    HIPCHK(ctx, r.d_pair.alloc(n_pairs));
    HIPCHK(ctx, r.d_mask.alloc(mask.size()));
    HIPCHK(ctx, r.d_wconst.alloc((size_t)16 * n_rep));
    HIPCHK(ctx, hipMemcpyAsync(r.d_ch, channel, sizeof(int) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(r.d_pair, pair_rep.data(), sizeof(int) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(r.d_mask, mask.data(), sizeof(unsigned long long) * mask.size(), hipMemcpyHostToDevice,
                               ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (the channel list is the caller's again, the host tables may go)
    return commit_set(*d, made, s);
}

// Speckled hold-out: replica k leaves out the entries (row, n) whose bit is set in held_out[(k rows_src + row) nw + (n >> 6)].
// The mask goes to the device as the caller packed it -- (n_rep rows_src, nw) is the row order of the replicated set.
extern "C" int vlgp_replicate_masked(vlgp_ctx* ctx, int src, int dst, int n_rep, const uint64_t* held_out) {
    UnitSet *s = nullptr, *d = nullptr;
    CHK(open_pair(ctx, src, dst, src == dst || n_rep < 1 || !held_out, "bad replicate arguments", &s, &d));
    CHK(replicas_check(ctx, src, dst, n_rep, s, d));
    // no bit at a channel >= N; whether two replicas hold the same entry out (vlgp_loglik then writes no rate)
    const int N = ctx->N, nw = (N + 63) / 64;
    const int64_t rs = s->rows;
    const uint64_t beyond = (N & 63) ? ~0ull << (N & 63) : 0ull;  // bits of the last word past channel N - 1
    std::vector<uint64_t> seen((size_t)rs * nw, 0ull);
    bool overlap = false;
    for (int k = 0; k < n_rep; ++k)
        for (int64_t r = 0; r < rs; ++r) {
            const uint64_t* mk = held_out + ((size_t)k * rs + r) * nw;
            if (mk[nw - 1] & beyond)
                return vlgp_fail(ctx, VLGP_ERR_ARG, "replica %d holds out a channel outside [0, %d) at row %lld", k, N,
                                 (long long)r);
            for (int q = 0; q < nw; ++q) {
                uint64_t& sw = seen[(size_t)r * nw + q];
                overlap = overlap || (sw & mk[q]) != 0;
                sw |= mk[q];
            }
        }
    UnitSet made;
    CHK(replicas_make(ctx, src, dst, n_rep, s, &made));
    Replicas& rp = made.rep;
    rp.by_row = true;
    rp.overlap = overlap;
    const size_t words = (size_t)n_rep * rs * nw;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "mask words are 64 bits");
    HIPCHK(ctx, rp.d_mask.alloc(words));
    if (ctx->n_gauss > 0) HIPCHK(ctx, rp.d_wconst.alloc((size_t)n_rep * rs * ctx->L));
    HIPCHK(ctx, hipMemcpyAsync(rp.d_mask, held_out, sizeof(uint64_t) * words, hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> nobs;  // one replica: a masked fit set, whose M-step divides by the observed rows of each channel
    if (n_rep == 1) {
        nobs.assign((size_t)N, (double)rs);
        for (int64_t r = 0; r < rs; ++r)
            for (int n = 0; n < N; ++n)
                if ((held_out[(size_t)r * nw + (n >> 6)] >> (n & 63)) & 1ull) nobs[n] -= 1.0;
        HIPCHK(ctx, rp.d_nobs.alloc((size_t)N));
        HIPCHK(ctx, hipMemcpyAsync(rp.d_nobs, nobs.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (the mask is the caller's again)
    return commit_set(*d, made, s);
}

// leave-one-out replicas: singleton groups
extern "C" int vlgp_replicate_units(vlgp_ctx* ctx, int src, int dst, int n_rep, const int* channel) {
    std::vector<int> start((size_t)(n_rep > 0 ? n_rep : 0) + 1);  // (n_rep < 1 is refused there, after the set checks)
    for (size_t k = 0; k < start.size(); ++k) start[k] = (int)k;
    return vlgp_replicate_groups(ctx, src, dst, n_rep, start.data(), channel);
}

// ---- parameters ------------------------------------------------------------
extern "C" int vlgp_set_params(vlgp_ctx* ctx, const double* a, const double* b, const double* noise) {
    NEED_CTX(ctx);
    CHK(vlgp_join_m(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    const int N = ctx->N, L = ctx->L, P = ctx->P;
    // through a pinned buffer of its own: the copies are truly asynchronous and nothing waits for them here (the E-step's
    // launches follow on the same stream); the buffer is reused only after the event behind the last copy has fired
    if (!ctx->h_stage_par) {
        HIPCHK(ctx, ctx->h_stage_par.alloc((size_t)(L + P) * N + N, hipHostMallocDefault));
        HIPCHK(ctx, hipEventCreateWithFlags(ctx->ev_stage_par.put(), hipEventDisableTiming));
    }
    if (ctx->stage_par_busy) HIPCHK(ctx, hipEventSynchronize(ctx->ev_stage_par));
    double* ha = ctx->h_stage_par;
    double* hb = ha + (size_t)L * N;
    double* hn = hb + (size_t)P * N;
    if (a) {
        memcpy(ha, a, sizeof(double) * L * N);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_a, ha, sizeof(double) * L * N, hipMemcpyHostToDevice, ctx->stream));
    }
    if (b) {
        memcpy(hb, b, sizeof(double) * P * N);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_b, hb, sizeof(double) * P * N, hipMemcpyHostToDevice, ctx->stream));
    }
    if (noise) {
        memcpy(hn, noise, sizeof(double) * N);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_noise, hn, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_stage_par, ctx->stream));
    ctx->stage_par_busy = true;
    ctx->msnap_valid = false;
    if (a && b && noise) ctx->have_params = true;
    return VLGP_OK;
}

extern "C" int vlgp_get_params(vlgp_ctx* ctx, double* a, double* b, double* noise, double* da, double* db) {
    NEED_CTX(ctx);
    CHK(vlgp_join_m(ctx));
    const int N = ctx->N, L = ctx->L, P = ctx->P;
    if (ctx->msnap_valid) {  // the M-step lane left them in pinned memory behind its last kernel (vlgp_mstep_begin)
        const double* h = ctx->h_msnap;
        const size_t ln[5] = {(size_t)L * N, (size_t)P * N, (size_t)N, (size_t)L * N, (size_t)P * N};
        double* out[5] = {a, b, noise, da, db};
        for (int i = 0; i < 5; ++i) {
            if (out[i]) memcpy(out[i], h, sizeof(double) * ln[i]);
            h += ln[i];
        }
        return VLGP_OK;
    }
    // five small copies into pageable memory are five synchronous staged transfers (~90 us per EM iteration): gather
    // them in the pinned buffer with truly asynchronous copies, one synchronisation, then hand them out
    double* dst[5] = {a, b, noise, da, db};
    const double* src[5] = {ctx->d_a, ctx->d_b, ctx->d_noise, ctx->d_da, ctx->d_db};
    const size_t len[5] = {(size_t)L * N, (size_t)P * N, (size_t)N, (size_t)L * N, (size_t)P * N};
    size_t total = 0;
    for (int i = 0; i < 5; ++i) total += dst[i] ? len[i] : 0;
    CHK(vlgp_ensure_pinned(ctx, (int64_t)total + 8));
    size_t o = 0;
    for (int i = 0; i < 5; ++i) {
        if (!dst[i]) continue;
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned + o, src[i], sizeof(double) * len[i], hipMemcpyDeviceToHost, ctx->stream));
        o += len[i];
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    o = 0;
    for (int i = 0; i < 5; ++i) {
        if (!dst[i]) continue;
        memcpy(dst[i], ctx->h_pinned + o, sizeof(double) * len[i]);
        o += len[i];
    }
    return VLGP_OK;
}

// ---- prior -----------------------------------------------------------------
static int rebuild_prior_table(vlgp_ctx* ctx) {
    CHK(vlgp_prior_collect(ctx));
    const int L = ctx->L;
    const int rows = (int)ctx->priors.size();
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->d_prior_base.reset(); ctx->d_prior_rl.reset(); ctx->d_prior_goff.reset();
    ctx->prior_rows = rows;
    ctx->prior_epoch++;
    if (rows == 0) return VLGP_OK;
    std::vector<const double*> base(rows);
    std::vector<int> rl(rows * L);
    std::vector<int64_t> goff(rows * L);
    int i = 0;
    for (auto& kv : ctx->priors) {
        Prior& pr = kv.second;
        pr.index = i;
        base[i] = pr.d_compact;
        for (int l = 0; l < L; ++l) {
            rl[i * L + l] = pr.rl[l];
            goff[i * L + l] = pr.goff[l];
        }
        ++i;
    }
    HIPCHK(ctx, ctx->d_prior_base.alloc(rows));
    HIPCHK(ctx, ctx->d_prior_rl.alloc((size_t)rows * L));
    HIPCHK(ctx, ctx->d_prior_goff.alloc((size_t)rows * L));
    HIPCHK(ctx, hipMemcpy(ctx->d_prior_base.get(), base.data(), sizeof(double*) * rows, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_prior_rl, rl.data(), sizeof(int) * rows * L, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_prior_goff, goff.data(), sizeof(int64_t) * rows * L, hipMemcpyHostToDevice));
    return VLGP_OK;
}

static int new_prior(vlgp_ctx* ctx, int T, Prior** out) {
    if (T < 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "prior length must be positive");
    auto it = ctx->priors.find(T);
    if (it != ctx->priors.end()) {
        *out = &it->second;
        return VLGP_OK;
    }
    Prior pr;
    pr.T = T;
    const int64_t n = (int64_t)ctx->L * T * ctx->R;
    HIPCHK(ctx, pr.d_full.alloc((size_t)n));
    HIPCHK(ctx, pr.d_compact.alloc((size_t)n));
    // capacity layout of the compact copy: latent l at l*T*R whatever the ranks turn out to be, so that the
    // factorisation kernel can write it (and the table never needs the ranks of the other latents)
    pr.goff.resize(ctx->L);
    for (int l = 0; l < ctx->L; ++l) pr.goff[l] = (int64_t)l * T * ctx->R;
    pr.compact_len = n;
    pr.rl.assign(ctx->L, 1);
    auto res = ctx->priors.emplace(T, std::move(pr));
    *out = &res.first->second;
    return VLGP_OK;
}

extern "C" int vlgp_clear_prior(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    free_priors(ctx);
    return rebuild_prior_table(ctx);
}

extern "C" int vlgp_build_prior(vlgp_ctx* ctx, int n_lengths, const int* lengths, const double* omega,
                                const double* sigma) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (n_lengths < 1 || !lengths || !omega || !sigma) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad build_prior arguments");
    CHK(vlgp_prior_collect(ctx));
    // the reference replaces the whole dict on every call (gp.py:158).  Same set of lengths as the table holds
    // (every H-step): the factors are rebuilt in place and the kernel refreshes the ranks of the table rows --
    // no allocation, no copy.  Otherwise: drop the lengths not listed, add the new ones, rebuild the table.
    bool same = (int)ctx->priors.size() > 0 && ctx->d_prior_rl != nullptr;
    for (int i = 0; same && i < n_lengths; ++i) same = ctx->priors.count(lengths[i]) > 0;
    for (auto it = ctx->priors.begin(); same && it != ctx->priors.end(); ++it)
        same = std::find(lengths, lengths + n_lengths, it->first) != lengths + n_lengths;
    if (!same) {
        for (auto it = ctx->priors.begin(); it != ctx->priors.end();) {
            if (std::find(lengths, lengths + n_lengths, it->first) == lengths + n_lengths) {
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                it = ctx->priors.erase(it);
            } else {
                ++it;
            }
        }
    }
    std::vector<Prior*> prs;
    for (int i = 0; i < n_lengths; ++i) {
        Prior* pr = nullptr;
        CHK(new_prior(ctx, lengths[i], &pr));
        if (std::find(prs.begin(), prs.end(), pr) == prs.end()) prs.push_back(pr);
    }
    // same lengths as the table holds (the rebuild of every EM iteration): nothing here needs the ranks on the host --
    // the next consumer of Prior::rl (an E-step dispatch, vlgp_get_prior) takes them
    CHK(launch_ichol_all(ctx, prs, omega, sigma, same, same));
    return same ? VLGP_OK : rebuild_prior_table(ctx);
}

extern "C" int vlgp_set_prior(vlgp_ctx* ctx, int T, const double* G) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (!G) return vlgp_fail(ctx, VLGP_ERR_ARG, "null G");
    CHK(vlgp_prior_collect(ctx));
    Prior* pr = nullptr;
    CHK(new_prior(ctx, T, &pr));
    const int64_t n = (int64_t)ctx->L * T * ctx->R;
    HIPCHK(ctx, hipMemcpyAsync(pr->d_full, G, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    CHK(launch_compact_prior(ctx, *pr));
    return rebuild_prior_table(ctx);
}

extern "C" int vlgp_get_prior(vlgp_ctx* ctx, int T, double* G, int* rank_out) {
    NEED_CTX(ctx);
    CHK(vlgp_prior_collect(ctx));
    auto it = ctx->priors.find(T);
    if (it == ctx->priors.end()) return vlgp_fail(ctx, VLGP_ERR_STATE, "no prior factor for length %d", T);
    const int64_t n = (int64_t)ctx->L * T * ctx->R;
    if (G) {
        HIPCHK(ctx, hipMemcpyAsync(G, it->second.d_full, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (rank_out)
        for (int l = 0; l < ctx->L; ++l) rank_out[l] = it->second.rl[l];
    return VLGP_OK;
}

int vlgp_bind_priors(vlgp_ctx* ctx, UnitSet& us) {
    if (us.prior_epoch == ctx->prior_epoch) return VLGP_OK;
    std::vector<int> idx(us.M);
    for (int m = 0; m < us.M; ++m) {
        const int T = (int)(us.off[m + 1] - us.off[m]);
        auto it = ctx->priors.find(T);
        if (it == ctx->priors.end())
            return vlgp_fail(ctx, VLGP_ERR_STATE, "no prior factor for unit length %d (call build_prior/set_prior)", T);
        idx[m] = it->second.index;
    }
    HIPCHK(ctx, hipMemcpy(us.d_unit_prior, idx.data(), sizeof(int) * us.M, hipMemcpyHostToDevice));
    us.prior_epoch = ctx->prior_epoch;
    return VLGP_OK;
}

int vlgp_refresh_xb(vlgp_ctx* ctx, UnitSet& us) {
    if (us.x_ones) return VLGP_OK;
    if (!us.d_xb) HIPCHK(ctx, us.d_xb.alloc((size_t)us.rows * ctx->N));
    return launch_xb(ctx, us);
}

// ---- E / M / H ---------------------------------------------------------------
static int begin_count(vlgp_ctx* ctx) {
    HIPCHK(ctx, hipMemsetAsync(ctx->d_fail, 0, sizeof(int), ctx->stream));
    return VLGP_OK;
}
static int end_count(vlgp_ctx* ctx, int* n_failed) {
    if (!n_failed) return VLGP_OK;
    HIPCHK(ctx, hipMemcpyAsync(n_failed, ctx->d_fail, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_update_w(vlgp_ctx* ctx, int set) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_COLLECT | OPEN_STALE | OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_update_w));
    return launch_estep(ctx, *us, EM_W, 0, 0.0, 0);
}

extern "C" int vlgp_update_v(vlgp_ctx* ctx, int set, int vb, int* n_failed) {
    UnitSet* us = nullptr;  // (no OPEN_STALE: v is not among what the H-step moments are built from)
    CHK(open_set(ctx, set, OPEN_COLLECT | OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_update_v));
    if (n_failed) *n_failed = 0;
    if (!vb) return VLGP_OK;
    CHK(begin_count(ctx));
    CHK(launch_estep(ctx, *us, EM_FACTOR0 | EM_V, 0, 0.0, 1));
    return end_count(ctx, n_failed);
}

// core.estep over overlapping segments, as the reference's sequential loop over VIEWS does it (vlgp/core.py:123-126 with
// vlgp/util.py:482-496): stage by stage; before a stage the shared rows (mu while it is still shared, v) come over from
// the previous stage's units, after it they go back, so that both copies of a shared row always hold what the
// reference's single row holds.  A stage is a contiguous range of equal-length units: a view of the set.
static int estep_staged(vlgp_ctx* ctx, UnitSet& us, int mode, int n_iter, double dmu_bound, int vb) {
    const int W = us.Tmax, N = ctx->N, L = ctx->L, P = ctx->P;
    CHK(vlgp_bind_priors(ctx, us));
    const int n_stages = (int)us.stage_start.size() - 1;
    for (int s = 0; s < n_stages; ++s) {
        const int u0 = us.stage_start[s], cnt = us.stage_start[s + 1] - u0;
        if (cnt < 1) continue;
        CHK(launch_links_copy(ctx, us, us.link_start[s], us.link_start[s + 1], 0));
        UnitSet v;
        v.valid = true; v.M = cnt; v.rows = (int64_t)cnt * W; v.Tmax = v.Tmin = W;
        v.off.resize(cnt + 1);
        for (int m = 0; m <= cnt; ++m) v.off[m] = (int64_t)m * W;
        v.d_off.borrow(us.d_off);  // 0, W, 2 W, ...: the first cnt + 1 entries serve any range of equal-length units
        const int64_t r0 = (int64_t)u0 * W;
        v.y.borrow(us.y + r0 * N); v.x.borrow(us.x ? us.x + r0 * P * N : nullptr);
        v.mu.borrow(us.mu + r0 * L); v.v.borrow(us.v + r0 * L); v.w.borrow(us.w + r0 * L); v.dmu.borrow(us.dmu + r0 * L);
        v.x_ones = us.x_ones; v.alias = true;  // (borrows everything)
        v.d_unit_prior.borrow(us.d_unit_prior + u0); v.prior_epoch = us.prior_epoch;
        if (!us.x_ones) {
            if (!us.d_xb) HIPCHK(ctx, us.d_xb.alloc((size_t)us.rows * N));
            v.d_xb.borrow(us.d_xb + r0 * N);
        }
        v.d_scratch = std::move(us.d_scratch);  // the stages run one after the other
        const int rc = launch_estep(ctx, v, mode, n_iter, dmu_bound, vb);
        us.d_scratch = std::move(v.d_scratch);  // (re)allocated inside: stays with the set
        if (rc != VLGP_OK) return rc;
        CHK(launch_links_copy(ctx, us, us.link_start[s], us.link_start[s + 1], 1));
    }
    return VLGP_OK;
}

extern "C" int vlgp_estep(vlgp_ctx* ctx, int set, int n_iter, double dmu_bound, int vb, int* n_failed) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_COLLECT | OPEN_STALE | OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_estep));
    if (n_failed) *n_failed = 0;
    if (n_iter < 1) return VLGP_OK;  // core.py:24-25
    if (!(dmu_bound > 0)) return vlgp_fail(ctx, VLGP_ERR_ARG, "dmu_bound must be positive");
    CHK(begin_count(ctx));
    const int mode = EM_FACTOR0 | EM_MEAN | EM_W | (vb ? EM_V : 0);
    if (us->stage_start.size() > 2) CHK(estep_staged(ctx, *us, mode, n_iter, dmu_bound, vb ? 1 : 0));
    else CHK(launch_estep(ctx, *us, mode, n_iter, dmu_bound, vb ? 1 : 0));
    if (!ctx->ev_e_done) HIPCHK(ctx, hipEventCreateWithFlags(ctx->ev_e_done.put(), hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(ctx->ev_e_done, ctx->stream));  // (vlgp_estep_wait: this call's launches, not what is queued behind)
    ctx->e_done_valid = true;
    return end_count(ctx, n_failed);
}

extern "C" int vlgp_set_overlaps(vlgp_ctx* ctx, int set, int n_stages, const int* stage_start, int n_links,
                                 const int* links, const int* link_start) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_set_overlaps));
    if (us->is(SET_TILING) || us->Tmin != us->Tmax)
        return vlgp_fail(ctx, VLGP_ERR_STATE, "overlaps belong to a copied cut of equal-length units");
    if (n_stages < 1 || !stage_start || stage_start[0] != 0 || stage_start[n_stages] != us->M || n_links < 0 ||
        (n_links > 0 && (!links || !link_start)))
        return vlgp_fail(ctx, VLGP_ERR_ARG, "bad overlap description");
    for (int s = 0; s < n_stages; ++s)
        if (stage_start[s + 1] < stage_start[s]) return vlgp_fail(ctx, VLGP_ERR_ARG, "stages must be ordered");
    for (int k = 0; k < n_links; ++k) {
        const int a = links[3 * k], b = links[3 * k + 1], o = links[3 * k + 2];
        if (a < 0 || a >= us->M || b < 0 || b >= us->M || a == b || o < 1 || o >= us->Tmax)
            return vlgp_fail(ctx, VLGP_ERR_ARG, "bad overlap link %d", k);
    }
    if (n_links > 0) {
        // link_start[s] .. link_start[s + 1] index `links` for stage s: they go to the copy kernels unchecked afterwards
        if (link_start[0] != 0 || link_start[n_stages] != n_links)
            return vlgp_fail(ctx, VLGP_ERR_ARG, "link_start must run from 0 to n_links");
        for (int s = 0; s < n_stages; ++s) {
            if (link_start[s + 1] < link_start[s]) return vlgp_fail(ctx, VLGP_ERR_ARG, "link_start must be non-decreasing");
            for (int k = link_start[s]; k < link_start[s + 1]; ++k) {
                const int b = links[3 * k + 1];  // the second unit of a link lies in the stage the link is filed under
                if (b < stage_start[s] || b >= stage_start[s + 1])
                    return vlgp_fail(ctx, VLGP_ERR_ARG, "overlap link %d is filed under stage %d but its second unit is not in it", k, s);
            }
        }
    }
    us->stage_start.assign(stage_start, stage_start + n_stages + 1);
    us->link_start.assign(n_links > 0 ? link_start : stage_start, (n_links > 0 ? link_start : stage_start) + n_stages + 1);
    if (n_links == 0) us->link_start.assign(n_stages + 1, 0);
    us->d_links.reset();
    us->n_links = n_links;
    us->share_mu = true;
    if (n_links > 0) {
        HIPCHK(ctx, us->d_links.alloc((size_t)3 * n_links));
        HIPCHK(ctx, hipMemcpy(us->d_links, links, sizeof(int) * 3 * n_links, hipMemcpyHostToDevice));
    }
    return VLGP_OK;
}

extern "C" int vlgp_unshare_mu(vlgp_ctx* ctx, int set) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, 0, &us, &admit_vlgp_unshare_mu));
    us->share_mu = false;
    return VLGP_OK;
}

extern "C" int vlgp_mstep_begin(vlgp_ctx* ctx, int set, int n_iter, int use_hessian, double eps, double lr,
                                double da_bound, double db_bound) {
    NEED_CTX(ctx);  // (an M-step in flight had its parameters: asking this first changes no answer)
    if (ctx->m_pending) return vlgp_fail(ctx, VLGP_ERR_STATE, "an M-step is already in flight (call vlgp_mstep_end)");
    UnitSet* us = nullptr;  // (no OPEN_JOIN: the call that starts the lane has nothing of it to wait for)
    CHK(open_set(ctx, set, OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_mstep_begin));
    if (!(da_bound > 0) || !(db_bound > 0)) return vlgp_fail(ctx, VLGP_ERR_ARG, "da_bound/db_bound must be positive");
    // fork: the M-step lane starts after everything already queued on the main stream
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->mstream, ctx->ev_fork, 0));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_fail_m, 0, sizeof(int), ctx->mstream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_m_start, ctx->mstream));
    ctx->msnap_valid = false;
    if (n_iter >= 1)  // core.py:131-133
        CHK(launch_mstep(ctx, *us, n_iter, use_hessian, eps, lr, da_bound, db_bound));
    {   // what the caller pulls afterwards (vlgp_get_params, the failure count), written out by the lane itself
        const int N = ctx->N, L = ctx->L, P = ctx->P;
        if (!ctx->h_msnap) {
            HIPCHK(ctx, ctx->h_msnap.alloc(2 * (size_t)(L + P) * N + N + 8, hipHostMallocMapped));
            CHK(device_view(ctx, ctx->d_msnap, ctx->h_msnap));
        }
        CHK(launch_snapshot_params(ctx, ctx->mstream, ctx->d_msnap));
        ctx->msnap_valid = true;  // (read only after vlgp_join_m; any vlgp_set_params in between clears it)
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_m_done, ctx->mstream));
    // NO device-side join here: the H-step rounds and the prior rebuild queued on the main stream meanwhile
    // touch neither a, b nor anything the M-step writes, and every entry point that does joins on the host
    // first (vlgp_join_m waits for ev_m_done) -- a stream wait here would serialise the H-step behind the M-step
    ctx->m_pending = true;
    return VLGP_OK;
}

extern "C" int vlgp_mstep_end(vlgp_ctx* ctx, int* n_failed, double* device_ms) {
    NEED_CTX(ctx);
    if (!ctx->m_pending) return vlgp_fail(ctx, VLGP_ERR_STATE, "no M-step in flight");
    CHK(vlgp_join_m(ctx));
    ctx->m_pending = false;
    {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev_m_start, ctx->ev_m_done));
        ctx->last_m_ms = ms;  // (vlgp_hstep_begin weighs it against the H-step bracket's duration)
        if (device_ms) *device_ms = ms;
    }
    if (n_failed) {
        if (ctx->msnap_valid) {
            const int N = ctx->N, L = ctx->L, P = ctx->P;
            memcpy(n_failed, ctx->h_msnap + 2 * (size_t)(L + P) * N + N, sizeof(int));
        } else {
            HIPCHK(ctx, hipMemcpy(n_failed, ctx->d_fail_m, sizeof(int), hipMemcpyDeviceToHost));
        }
    }
    return VLGP_OK;
}

extern "C" int vlgp_mstep(vlgp_ctx* ctx, int set, int n_iter, int use_hessian, double eps, double lr,
                          double da_bound, double db_bound, int* n_failed) {
    NEED_CTX(ctx);
    if (n_failed) *n_failed = 0;
    if (n_iter < 1) return VLGP_OK;  // core.py:131-133
    CHK(vlgp_mstep_begin(ctx, set, n_iter, use_hessian, eps, lr, da_bound, db_bound));
    return vlgp_mstep_end(ctx, n_failed, nullptr);
}

// core.mstep under a full covariance per row (mstep_cov.hip).  Opens as an entry point that writes
// parameters; every refusal comes before the first launch that writes one: the admission, the limits and arguments
// (mstep_cov_refusal, call_block.h), then a pass over the uploaded moments for a non-finite value.
// (the part vlgp_mstep_cov and vlgp_mstep_cov_masked share: the set is admitted and the arguments are checked)
static int mstep_cov_run(vlgp_ctx* ctx, const char* who, UnitSet* us, const double* mu, const double* cov, int n_iter,
                         int use_hessian, double eps, double lr, double da_bound, double db_bound, int* n_failed) {
    if (!(da_bound > 0) || !(db_bound > 0)) return vlgp_fail(ctx, VLGP_ERR_ARG, "da_bound/db_bound must be positive");
    const int64_t rows = us->rows;
    const int L = ctx->L;
    const MstepCovLayout o = mstep_cov_layout(rows, L);
    hipStream_t st = ctx->mstream;
    HIPCHK(ctx, ctx->d_mcov.ensure(o.need, o.need + o.need / 4 + 1024, st));
    // the M-step lane starts after everything already queued on the main stream
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_fork, 0));
    double* B = ctx->d_mcov;
    unsigned long long first = (unsigned long long)rows;
    unsigned long long* d_first = reinterpret_cast<unsigned long long*>(B + o.first);
    HIPCHK(ctx, hipMemcpyAsync(d_first, &first, sizeof(first), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(B + o.mu, mu, sizeof(double) * (size_t)(rows * L), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(B + o.cov, cov, sizeof(double) * (size_t)(o.need - o.cov), hipMemcpyHostToDevice, st));
    CHK(launch_mcov_first_bad_row(ctx, rows, B + o.mu, B + o.cov, d_first, st));
    HIPCHK(ctx, hipMemcpyAsync(&first, d_first, sizeof(first), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (first < (unsigned long long)rows)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: mu or cov of row %lld is not finite (the rows of a unit whose "
                         "Newton iteration failed?)", who, (long long)first);
    HIPCHK(ctx, hipMemsetAsync(ctx->d_fail_m, 0, sizeof(int), st));
    ctx->msnap_valid = false;
    CHK(launch_mstep_cov(ctx, *us, B + o.mu, B + o.cov, n_iter, use_hessian, eps, lr, da_bound, db_bound));
    int nf = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nf, ctx->d_fail_m, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (n_failed) *n_failed = nf;
    return VLGP_OK;
}
extern "C" int vlgp_mstep_cov(vlgp_ctx* ctx, int set, const double* mu, const double* cov, int n_iter, int use_hessian,
                              double eps, double lr, double da_bound, double db_bound, int* n_failed) {
    NEED_CTX(ctx);
    if (n_failed) *n_failed = 0;
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_mstep_cov));
    const MstepCovRefusal r = mstep_cov_refusal(ctx->L, ctx->P, ctx->sw.mstep_generic, ctx->world, mu, cov, n_iter);
    if (r.status) return vlgp_fail(ctx, r.status, "%s", r.text);
    return mstep_cov_run(ctx, "vlgp_mstep_cov", us, mu, cov, n_iter, use_hessian, eps, lr, da_bound, db_bound, n_failed);
}
// ... of a masked fit set: every channel over its observed rows.  The same frame and the same order of
// refusals, the Gaussian channel first among the limits (mstep_cov_masked_refusal).
extern "C" int vlgp_mstep_cov_masked(vlgp_ctx* ctx, int set, const double* mu, const double* cov, int n_iter, int use_hessian,
                                     double eps, double lr, double da_bound, double db_bound, int* n_failed) {
    NEED_CTX(ctx);
    if (n_failed) *n_failed = 0;
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, &admit_vlgp_mstep_cov_masked));
    const MstepCovRefusal r = mstep_cov_masked_refusal(ctx->n_gauss, ctx->L, ctx->P, ctx->sw.mstep_generic, ctx->world, mu,
                                                       cov, n_iter);
    if (r.status) return vlgp_fail(ctx, r.status, "%s", r.text);
    return mstep_cov_run(ctx, "vlgp_mstep_cov_masked", us, mu, cov, n_iter, use_hessian, eps, lr, da_bound, db_bound, n_failed);
}

extern "C" int vlgp_hstep_objective(vlgp_ctx* ctx, int set, int window, double dt, int n_eval, const int* latent,
                                    const double* logp, double* ll, double* dll) {
    UnitSet* us = nullptr;  // (no OPEN_JOIN: it runs beside the M-step lane)
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_hstep_objective));
    if (n_eval < 1 || !latent || !logp || !ll || !dll) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad hstep arguments");
    return launch_hstep(ctx, *us, window, dt, n_eval, latent, logp, ll, dll);
}

extern "C" int vlgp_hstep_prepare(vlgp_ctx* ctx, int set, int window) {
    UnitSet* us = nullptr;  // (no OPEN_JOIN: it runs beside the M-step lane)
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_hstep_prepare));
    ctx->hprep = false;
    if (ctx->hmom_bracket || window < 1) return VLGP_OK;
    // On the MAIN stream, behind everything queued so far -- the call may come while the E-step still runs (the host
    // then waits for the E-step alone: vlgp_estep_wait).  (Measured: the same work on the side stream, enqueued during the
    // E-step, makes a fourth busy queue beside the E-step's two lanes and the M-step lane -- E-step 2.2 -> 4.0 ms, the
    // queue pathology of DESIGN 4.1.)
    CHK(hstep_prepare(ctx, *us, window, ctx->stream));
    ctx->hprep = ctx->hmom_us == us;
    ctx->hprep_epoch = ctx->write_epoch;
    return VLGP_OK;
}

extern "C" int vlgp_hstep_begin(vlgp_ctx* ctx, int set, int window) {
    UnitSet* us = nullptr;  // (host bookkeeping only: no wait, no device call)
    CHK(open_set(ctx, set, 0, &us, &admit_vlgp_hstep_begin));
    ctx->hmom_bracket = true;
    // the first objective call inside the bracket builds the moments and the w copy -- unless vlgp_hstep_prepare did,
    // for this set and window, and no entry point that may change the units ran since
    if (!(ctx->hprep && ctx->hprep_epoch == ctx->write_epoch && ctx->hmom_us == us && ctx->hmom_T == window)) {
        ctx->hmom_us = nullptr;
        ctx->hwlm_valid = false;
    }
    ctx->hprep = false;
    // the rounds' waves take the high instruction priority unless the M-step lane was the longer one last time
    ctx->h_prio = (ctx->last_m_ms > 0.0 && ctx->last_h_ms > 0.0 && ctx->last_m_ms > ctx->last_h_ms) ? 0 : 1;
    ctx->h_t0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    return VLGP_OK;
}

extern "C" int vlgp_hstep_end(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    if (ctx->hmom_bracket && ctx->h_t0 > 0.0)
        ctx->last_h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - ctx->h_t0;
    ctx->hmom_bracket = false;
    ctx->hmom_us = nullptr;
    ctx->hwlm_valid = false;
    return VLGP_OK;
}

// ---- constraints / norms -----------------------------------------------------
extern "C" int vlgp_apply_latent_map(vlgp_ctx* ctx, int set, const double* map, const double* shift) {
    NEED_CTX(ctx);
    ctx->hmom_us = nullptr;  // unit state changes: cached H-step moments are stale
    CHK(vlgp_join_m(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    UnitSet* us = vlgp_get_set(ctx, set, true);
    if (!us || !map) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad latent map arguments");
    CHK(admit(ctx, set, us, admit_vlgp_apply_latent_map));
    const int L = ctx->L;
    // staged through a pinned and a device buffer of its own, reused after the event behind the last kernel that read
    // them: nothing waits here (this is the first call of every EM iteration, constrain_loading)
    if (!ctx->h_stage_map) {
        HIPCHK(ctx, ctx->h_stage_map.alloc((size_t)L * L + L + 8, hipHostMallocDefault));
        HIPCHK(ctx, ctx->d_stage_map.alloc((size_t)L * L + L + 8));
        HIPCHK(ctx, hipEventCreateWithFlags(ctx->ev_stage_map.put(), hipEventDisableTiming));
    }
    if (ctx->stage_map_busy) HIPCHK(ctx, hipEventSynchronize(ctx->ev_stage_map));
    memcpy(ctx->h_stage_map, map, sizeof(double) * L * L);
    if (shift) memcpy(ctx->h_stage_map + L * L, shift, sizeof(double) * L);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage_map, ctx->h_stage_map, sizeof(double) * (L * L + L), hipMemcpyHostToDevice, ctx->stream));
    const double* d_map = ctx->d_stage_map;
    const double* d_shift = shift ? ctx->d_stage_map + L * L : nullptr;
    CHK(launch_latent_map(ctx, *us, d_map, d_shift));
    // the set's units are independent copies: an IN-PLACE constraint of the reference (everything but "svd", which
    // rebinds mu) visits a row shared by two overlapping segments twice -- the caller says so with vlgp_unshare_mu
    CHK(launch_links_map(ctx, *us, d_map, d_shift));
    HIPCHK(ctx, hipEventRecord(ctx->ev_stage_map, ctx->stream));
    ctx->stage_map_busy = true;
    return VLGP_OK;
}

static int moments_host(vlgp_ctx* ctx, UnitSet& us, std::vector<double>& out) {
    const int L = ctx->L;
    const int K = L * (L + 1) / 2 + 3 * L + 1;
    CHK(vlgp_ensure_pinned(ctx, K + 8));
    CHK(launch_moments(ctx, us));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctx->d_work, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    out.assign(ctx->h_pinned.get(), ctx->h_pinned + K);
    return VLGP_OK;
}

extern "C" int vlgp_norms_begin(vlgp_ctx* ctx, int set);
extern "C" int vlgp_norms_end(vlgp_ctx* ctx, double out[2]);
extern "C" int vlgp_norms(vlgp_ctx* ctx, int set, double out[2]) {
    UnitSet* us = nullptr;  // (no OPEN_JOIN: it runs beside the M-step lane)
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_norms));
    if (ctx->world == 1) {  // one rank: the kernel of the two-halves form (the same sums, bit for bit)
        CHK(vlgp_norms_begin(ctx, set));
        return vlgp_norms_end(ctx, out);
    }
    std::vector<double> m;
    CHK(moments_host(ctx, *us, m));
    const int L = ctx->L, t = L * (L + 1) / 2;
    double s = 0.0;
    for (int l = 0; l < L; ++l) s += m[t + 2 * L + l];
    out[0] = s;
    out[1] = m[t + 3 * L];
    return VLGP_OK;
}

extern "C" int vlgp_norms_begin(vlgp_ctx* ctx, int set) {
    UnitSet* us = nullptr;  // (no OPEN_JOIN: it runs beside the M-step lane)
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_norms_begin));
    CHK(wait_norms(ctx));  // (a pass never collected: dropped)
    ctx->x_pending = 0;
    ctx->x_set = set;
    if (ctx->world > 1) {  // the sums cross ranks on the main lane's communicator: computed when they are collected
        ctx->x_pending = 2;
        return VLGP_OK;
    }
    if (!ctx->h_xres) {
        HIPCHK(ctx, ctx->d_xwork.alloc(2 * 1024 + 8));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_xwork, 0, sizeof(double) * (2 * 1024 + 8), ctx->stream));
        HIPCHK(ctx, ctx->h_xres.alloc(8, hipHostMallocMapped));
        memset(ctx->h_xres, 0, sizeof(double) * 8);
        CHK(device_view(ctx, ctx->d_xres, ctx->h_xres));
    }
    ++ctx->x_seq;
    CHK(launch_norms(ctx, *us, ctx->d_xwork, reinterpret_cast<unsigned*>(ctx->d_xwork + 2 * 1024), ctx->d_xres, ctx->x_seq));
    ctx->x_pending = 1;
    return VLGP_OK;
}

extern "C" int vlgp_norms_end(vlgp_ctx* ctx, double out[2]) {
    NEED_CTX(ctx);
    if (!ctx->x_pending) return vlgp_fail(ctx, VLGP_ERR_STATE, "no norms pass pending (vlgp_norms_begin)");
    if (ctx->x_pending == 2) {
        ctx->x_pending = 0;
        return vlgp_norms(ctx, ctx->x_set, out);
    }
    CHK(wait_norms(ctx));
    ctx->x_pending = 0;
    out[0] = ctx->h_xres[0];
    out[1] = ctx->h_xres[1];
    return VLGP_OK;
}

extern "C" int vlgp_latent_moments(vlgp_ctx* ctx, int set, double* sum1, double* sum2, double* count) {
    UnitSet* us = nullptr;  // (no OPEN_JOIN: it runs beside the M-step lane)
    CHK(open_set(ctx, set, OPEN_DEVICE, &us, &admit_vlgp_latent_moments));
    std::vector<double> m;
    CHK(moments_host(ctx, *us, m));
    const int L = ctx->L, t = L * (L + 1) / 2;
    for (int l = 0; l < L; ++l) {
        if (sum1) sum1[l] = m[t + l];
        if (sum2) sum2[l] = m[t + 2 * L + l];
    }
    if (count) {
        double c = (double)us->rows;
        if (ctx->world > 1) {
            CHK(vlgp_ensure_work(ctx, 8));
            HIPCHK(ctx, hipMemcpy(ctx->d_work, &c, sizeof(double), hipMemcpyHostToDevice));
            CHK(vlgp_allreduce(ctx, LANE_MAIN, ctx->d_work, 1));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            HIPCHK(ctx, hipMemcpy(&c, ctx->d_work, sizeof(double), hipMemcpyDeviceToHost));
        }
        *count = c;
    }
    return VLGP_OK;
}

extern "C" int vlgp_project_units(vlgp_ctx* ctx, int set, const double* proj, const double* shift, double* colsum) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_STALE | OPEN_JOIN | OPEN_DEVICE, &us, &admit_vlgp_project_units));
    if (!proj || !shift) return vlgp_fail(ctx, VLGP_ERR_ARG, "null projection");
    if (us->is(SET_TILING)) return vlgp_fail(ctx, VLGP_ERR_STATE, "project the owning set, not an aliased cut");
    const int N = ctx->N, L = ctx->L;
    const int64_t G = (us->rows + 63) / 64;
    const int64_t o_proj = 0, o_shift = (int64_t)N * L, o_out = o_shift + L + (L & 1), o_part = o_out + N + (N & 1);
    CHK(vlgp_ensure_work(ctx, o_part + G * N));
    CHK(vlgp_ensure_pinned(ctx, o_out + N + 8));
    memcpy(ctx->h_pinned, proj, sizeof(double) * N * L);
    memcpy(ctx->h_pinned + o_shift, shift, sizeof(double) * L);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_work, ctx->h_pinned, sizeof(double) * (o_shift + L), hipMemcpyHostToDevice,
                               ctx->stream));
    CHK(launch_project(ctx, *us, ctx->d_work + o_proj, ctx->d_work + o_shift, ctx->d_work + o_part,
                       ctx->d_work + o_out));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned + o_out, ctx->d_work + o_out, sizeof(double) * N, hipMemcpyDeviceToHost,
                               ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (colsum) memcpy(colsum, ctx->h_pinned + o_out, sizeof(double) * N);
    return VLGP_OK;
}

// ---- posterior draws -----------------------------------------------------------
extern "C" int vlgp_sample_posterior(vlgp_ctx* ctx, int T, const double* mu, const double* w, const double* G, int nsamples,
                                     const double* eps, double* out, int* n_failed) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (T < 1 || nsamples < 1 || !mu || !w || !G || !eps || !out) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad sample_posterior arguments");
    const int L = ctx->L, R = ctx->R;
    const int64_t n_mu = (int64_t)T * L, n_G = (int64_t)L * T * R, n_eps = (int64_t)L * R * nsamples;
    const int64_t n_out = (int64_t)nsamples * T * L;
    const int64_t o_mu = 0, o_w = o_mu + n_mu, o_G = o_w + n_mu, o_eps = o_G + n_G, o_z = o_eps + n_eps, o_out = o_z + n_eps;
    CHK(vlgp_ensure_work(ctx, o_out + n_out));
    double* W = ctx->d_work;
    if (n_failed) *n_failed = 0;
    CHK(begin_count(ctx));
    HIPCHK(ctx, hipMemcpyAsync(W + o_mu, mu, sizeof(double) * n_mu, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W + o_w, w, sizeof(double) * n_mu, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W + o_G, G, sizeof(double) * n_G, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W + o_eps, eps, sizeof(double) * n_eps, hipMemcpyHostToDevice, ctx->stream));
    CHK(launch_sample_posterior(ctx, T, nsamples, W + o_mu, W + o_w, W + o_G, W + o_eps, W + o_z, W + o_out));
    HIPCHK(ctx, hipMemcpyAsync(out, W + o_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return end_count(ctx, n_failed);
}

// ---- measurement -------------------------------------------------------------
extern "C" int vlgp_debug_last_estep_path(vlgp_ctx* ctx, int* path) {
    NEED_CTX(ctx);
    if (!path) return vlgp_fail(ctx, VLGP_ERR_ARG, "null path");
    *path = ctx->last_estep_path;
    return VLGP_OK;
}

// One value of the table VLGP_SWITCHES (ctx.h) from the environment; `warned`: that switch was reported already.
enum SwKind { SW_FLAG, SW_TRI, SW_INT, SW_REAL };
static double read_switch(const char* name, SwKind kind, double def, double lo, double hi, bool* warned) {
    const char* s = getenv(name);
    if (kind == SW_FLAG) return s != nullptr;
    if (!s) return def;
    if (kind == SW_TRI && (s[0] == '0' || s[0] == '1')) return s[0] - '0';
    if (kind == SW_INT || kind == SW_REAL) {
        char* end = nullptr;
        const double v = kind == SW_INT ? (double)strtol(s, &end, 10) : strtod(s, &end);
        if (end != s && *end == '\0' && (kind == SW_INT ? v >= lo : v > lo) && v <= hi) return v;
    }
    if (!*warned) fprintf(stderr, "vlgp: %s=\"%s\" is malformed or out of range: the default holds\n", name, s);
    *warned = true;
    return def;
}

void vlgp_read_switches(vlgp_ctx* ctx) {
    Switches& w = ctx->sw;
#define X(name, field, kind, def, lo, hi, what)                                                        \
    {                                                                                                  \
        static bool warned = false;                                                                    \
        w.field = (VLGP_SW_T_##kind)read_switch(name, SW_##kind, (double)(def), (double)(lo), (double)(hi), &warned); \
    }
    VLGP_SWITCHES(X)
#undef X
}

extern "C" int vlgp_debug_reload_switches(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    vlgp_read_switches(ctx);
    return VLGP_OK;
}

extern "C" int vlgp_debug_switch(vlgp_ctx* ctx, const char* name, double* value) {
    NEED_CTX(ctx);
    if (!name || !value) return vlgp_fail(ctx, VLGP_ERR_ARG, "null switch name or value");
#define X(sname, field, kind, def, lo, hi, what) \
    if (!strcmp(name, sname)) { *value = (double)ctx->sw.field; return VLGP_OK; }
    VLGP_SWITCHES(X)
#undef X
    return vlgp_fail(ctx, VLGP_ERR_ARG, "unknown switch %s", name);
}

extern "C" int vlgp_debug_last_hstep_path(vlgp_ctx* ctx, int* path) {
    NEED_CTX(ctx);
    if (!path) return vlgp_fail(ctx, VLGP_ERR_ARG, "null path");
    *path = ctx->last_hstep_path;
    return VLGP_OK;
}

extern "C" int vlgp_debug_hstep_stats(vlgp_ctx* ctx, double out[4]) {
    NEED_CTX(ctx);
    if (!out) return vlgp_fail(ctx, VLGP_ERR_ARG, "null out");
    for (int i = 0; i < 4; ++i) out[i] = ctx->hstat[i];
    return VLGP_OK;
}

extern "C" int vlgp_debug_hstep_plan(vlgp_ctx* ctx, int out[VLGP_HSTEP_PLAN_LEN]) {
    NEED_CTX(ctx);
    if (!out) return vlgp_fail(ctx, VLGP_ERR_ARG, "null out");
    for (int i = 0; i < VLGP_HSTEP_PLAN_LEN; ++i) out[i] = ctx->hplan[i];
    return VLGP_OK;
}

extern "C" int vlgp_debug_mstep_plan(vlgp_ctx* ctx, int64_t rows, int out[12]) {
    NEED_CTX(ctx);
    if (rows < 1 || !out) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad plan arguments");
    return mstep_plan_report(ctx, rows, out);
}

extern "C" int vlgp_debug_estep_plan(vlgp_ctx* ctx, int set, int mode, int n_iter, int out[VLGP_ESTEP_PLAN_LEN]) {
    NEED_CTX(ctx);
    if (!out || n_iter < 0 || mode < 1 || mode > (EM_FACTOR0 | EM_MEAN | EM_W | EM_V))
        return vlgp_fail(ctx, VLGP_ERR_ARG, "bad plan arguments");
    CHK(vlgp_prior_collect(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    UnitSet* us = vlgp_get_set(ctx, set, true);
    if (!us) return VLGP_ERR_ARG;
    // (vlgp_estep runs a staged set through launch_estep once per stage view: lengths, lanes and cuts differ per stage)
    if (us->stage_start.size() > 2)
        return vlgp_fail(ctx, VLGP_ERR_STATE, "set %d is staged (vlgp_set_overlaps): there is one plan per stage, not one for the set", set);
    for (int i = 0; i < VLGP_ESTEP_PLAN_LEN; ++i) out[i] = 0;
    return launch_estep(ctx, *us, mode, n_iter, 1.0, (mode & EM_V) != 0, out);
}

extern "C" int vlgp_debug_npx(vlgp_ctx* ctx, int kind, int64_t n, const double* a, const double* b, double* out) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->dev));
    if (n < 1 || !a || !out || kind < 0 || kind > 8 || ((kind == 2 || kind == 3) && !b)) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad probe arguments");
    CHK(vlgp_ensure_work(ctx, 3 * n));
    double* W = ctx->d_work;
    HIPCHK(ctx, hipMemcpyAsync(W, a, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    if (b) HIPCHK(ctx, hipMemcpyAsync(W + n, b, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(W + 2 * n, out, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    CHK(launch_npx_probe(ctx, kind, n, W, W + n, W + 2 * n));
    HIPCHK(ctx, hipMemcpyAsync(out, W + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VLGP_OK;
}

extern "C" int vlgp_debug_phase_clock(vlgp_ctx* ctx, int on, uint64_t out[8]) {
    NEED_CTX(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (out) {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        if (ctx->d_clk) HIPCHK(ctx, hipMemcpy(out, ctx->d_clk, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (on) {
        if (!ctx->d_clk) HIPCHK(ctx, ctx->d_clk.alloc(8));
        HIPCHK(ctx, hipMemset(ctx->d_clk, 0, 8 * sizeof(uint64_t)));
    } else {
        ctx->d_clk.reset();
    }
    return VLGP_OK;
}

extern "C" int vlgp_profile_enable(vlgp_ctx* ctx, int on) {
    NEED_CTX(ctx);
    if (!on) prof_drain(ctx);
    ctx->prof_on = on != 0;
    return VLGP_OK;
}
extern "C" int vlgp_profile_reset(vlgp_ctx* ctx) {
    NEED_CTX(ctx);
    prof_drain(ctx);
    for (auto& p : ctx->prof) p = ProfSlot();
    return VLGP_OK;
}
extern "C" int vlgp_profile_get(vlgp_ctx* ctx, int kind, int64_t* launches, double* total_ms, double* units) {
    NEED_CTX(ctx);
    if (kind < 0 || kind >= VLGP_PROF_KINDS) return vlgp_fail(ctx, VLGP_ERR_ARG, "bad profile kind %d", kind);
    prof_drain(ctx);
    ProfSlot tot = ctx->prof[kind];
    if (kind == VLGP_PROF_ESTEP)  // every E-step kernel, whichever instantiation ran
        for (int k = VLGP_PROF_ESTEP_RA16; k <= VLGP_PROF_ESTEP_GENERIC; ++k) {
            tot.launches += ctx->prof[k].launches;
            tot.ms += ctx->prof[k].ms;
            tot.units += ctx->prof[k].units;
        }
    if (launches) *launches = tot.launches;
    if (total_ms) *total_ms = tot.ms;
    if (units) *units = tot.units;
    return VLGP_OK;
}
