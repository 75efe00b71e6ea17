// Internal state behind the opaque vlgp_ctx handle (host side, C++17).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/vlgp_hip.h"
#include "dev_mem.h"

#define VLGP_WAVE 64
#define VLGP_E_LANES 4          // split E-step: the unit set runs as up to this many independent lanes (streams)
#define VLGP_PRIOR_SLOTS 64   // prior lengths factored per mailbox round

// One low-rank prior factor per distinct unit length (gp.make_cholesky).
struct Prior {
    int T = 0;
    DevPtr<double> d_full;        // (L, T, R) as the reference lays it out
    DevPtr<double> d_compact;     // per latent: (T, rl) row-major, zero columns dropped
    std::vector<int> rl;          // effective rank per latent
    std::vector<int64_t> goff;    // offset of latent l inside d_compact (doubles)
    int64_t compact_len = 0;
    int index = -1;               // row in the device prior table
};

// The kinds of unit set, one bit each, and the masks the host code asks for (api.hip holds the table of which
// entry point takes which kinds).
enum : unsigned {
    SET_PLAIN = 1,        // uploaded (vlgp_upload_units)
    SET_TILING = 2,       // a cut whose windows tile the source: shares y / x / mu / v / w with `parent` (alias)
    SET_COPIED = 4,       // a cut with rows of its own, with or without overlaps (vlgp_set_overlaps)
    SET_GROUPS = 8,       // replicas that leave groups of channels out (vlgp_replicate_groups / _units)
    SET_MASKED = 16,      // replicas that leave single entries out (vlgp_replicate_masked), two or more of them
    SET_MASKED_FIT = 32,  // ... exactly one: the source's rows with a mask, the set a fit with missing observations runs on
    SET_REPLICATED = SET_GROUPS | SET_MASKED | SET_MASKED_FIT,
    SET_BY_ROW = SET_MASKED | SET_MASKED_FIT,                    // one mask per row, not one per replica
    SET_FIT = SET_PLAIN | SET_TILING | SET_COPIED | SET_MASKED_FIT,  // the fit (update_w / v, M-step, H-step, norms) may run on it
    SET_SOURCE = 64,      // admission only: the call also takes a set that is the source of replicas
    SET_ANY = 127,
};

// Replicated set (vlgp_replicate_groups; vlgp_replicate_units = singleton groups): n copies of set src's units,
// replica-major (unit k M_src + m), replica k leaving a group of channels out of its E-step.  The n_pairs (replica,
// left-out channel) pairs are listed in the caller's order: pair p is channel d_ch[p] of replica d_pair[p].  The
// E-step reads the groups as bit masks, nw = (N + 63) / 64 words per replica, bit n & 63 of word n >> 6 set when
// the replica leaves channel n out.  y and xb are the source's (aliased, never freed here); mu, v, w, dmu are the
// replicas' own.  The source counts the replica sets that alias it (UnitSet::rep_users) and refuses re-upload / free.
// A masked set (vlgp_replicate_masked) is the general form, one mask per ROW: by_row, d_mask (n rows_src, nw) indexed by
// the replicated row, d_wconst (n rows_src, L) or null without a Gaussian channel, no pairs (n_pairs == 0); overlap:
// some (row, channel) is held out by more than one replica (decided on the host when the set is made: vlgp_loglik then
// has no single replica to write that entry's rate from).
struct Replicas {
    int src = -1;                 // the set whose y / x / xb rows these are; -1: not a replicated set
    bool by_row = false, overlap = false;
    int n = 0, n_pairs = 0, nw = 0;
    int64_t rows_src = 0;
    DevPtr<int> d_ch;             // groups: (n_pairs) left-out channel of each pair
    DevPtr<int> d_pair;           // groups: (n_pairs) replica of each pair
    DevPtr<unsigned long long> d_mask;  // groups (n, nw), by_row (n rows_src, nw): membership masks
    DevPtr<double> d_wconst;      // Gaussian constant of w (estep_split.hip): groups (n, 16) per replica, by_row per row
    DevPtr<double> d_nobs;        // by_row with n == 1 only: (N) observed rows per channel (M-step noise)
    DevPtr<double> d_xa;          // the replica table of the row passes (estep_split.hip, ExclArgs), and its host copy
    double xh[8] = {};
};

// Move-only: every device pointer is an owner (dev_mem.h).  What a set borrows instead of owning, by kind:
// a tiling cut y, x, mu, v, w of its parent; a replicated set y, x and (launch_estep) d_xb of its source; the view of
// one stage that estep_staged builds everything.
struct UnitSet {
    bool valid = false;
    int M = 0;
    int64_t rows = 0;
    int Tmax = 0, Tmin = 0;
    std::vector<int64_t> off;     // host copy of offsets (M+1)
    DevPtr<int64_t> d_off;
    DevPtr<double> y, x, mu, v, w, dmu;
    bool x_ones = true;
    bool alias = false;           // shares y/x/mu/v/w with `parent` (exact tiling cut)
    int parent = -1;
    std::vector<int64_t> src_start;  // for non-aliased cuts: source row of each unit
    DevPtr<int64_t> d_src_start;
    DevPtr<int> d_unit_prior;     // prior-table row per unit
    uint64_t prior_epoch = 0;     // epoch of the table d_unit_prior was built against
    DevPtr<double> d_xb;          // (rows, N) x.b, only when !x_ones
    DevPtr<double> d_mu_stash;    // copy of mu taken by vlgp_stash_mu (rows x L)
    GrowBuf<double> d_scratch;    // E-step scratch (generic, long-unit and split families)
    double rows_all_ranks = 0.0;  // sum of `rows` over the ranks (M-step noise), exchanged on first use; 0 = unknown
    // Overlapping segments of a non-aliased cut (trial lengths that are not multiples of the window, vlgp/util.py:482-496).
    // In the reference they are VIEWS of the same trial rows: segment k + 1 starts its E-step from the mu, v that segment k
    // left in the shared rows, and an in-place constraint touches a shared row once per segment that holds it.  Here the
    // units are independent copies stored STAGE-MAJOR (stage = position in a chain of overlapping neighbours), the E-step
    // runs stage by stage and the shared rows are copied forward before and back after each stage (vlgp_set_overlaps).
    std::vector<int> stage_start;   // unit index of the first unit of each stage, + M at the end; empty: no overlaps
    std::vector<int> link_start;    // per stage s: links [link_start[s], link_start[s + 1]) have their second unit in s
    DevPtr<int> d_links;            // (n_links, 3): first unit, second unit, shared rows
    int n_links = 0;
    bool share_mu = true;           // false once the segments' mu was rebound (constrain_loading "svd")
    Replicas rep;                   // what a replicated set holds beside its own mu, v, w, dmu (default: not replicated)
    int rep_users = 0;              // replicated sets whose y / x / xb are this set's rows

    // What kind of set this is: exactly one SET_* bit.  Every question the host code asks about a set is a
    // mask of kinds: us.is(SET_REPLICATED), us.is(SET_BY_ROW), us.is(SET_FIT).
    unsigned kind() const {
        if (rep.src >= 0) return !rep.by_row ? SET_GROUPS : (rep.n == 1 ? SET_MASKED_FIT : SET_MASKED);
        return alias ? SET_TILING : (parent >= 0 ? SET_COPIED : SET_PLAIN);
    }
    bool is(unsigned kinds) const { return (kind() & kinds) != 0; }
    bool is_source() const { return rep_users > 0; }  // replicas alias its rows: no re-upload, no free, no new contents
};

// Every debug / test switch the library reads from the environment, ONE table: X(name, field, kind, default, lo, hi, what).
// Kinds: FLAG  on when the variable is set, whatever its value;
//        TRI   -1 unset, 0 / 1 by the first character of the value;
//        INT   lo <= value <= hi;   REAL  lo < value <= hi.
// A malformed or out-of-range value is reported on stderr (once per switch) and the default holds.  One lifetime for
// all of them: vlgp_read_switches fills vlgp_ctx::sw when the handle is created and again on
// vlgp_debug_reload_switches; nothing else reads the environment (the communicator set-up apart): no launch pays for it.
#define VLGP_SWITCHES(X)                                                                                                 \
    X("VLGP_ESTEP_SPLIT", estep_split, TRI, -1, 0, 1, "split E-step (chip-wide launches per phase): 0 never, 1 whatever the set's size") \
    X("VLGP_ESTEP_LSPLIT", estep_lsplit, TRI, -1, 0, 1, "long units (T > 64) on the split E-step: 0 never, 1 below 128 tasks too") \
    X("VLGP_ESTEP_GENERIC", estep_generic, FLAG, false, 0, 1, "E-step: the generic kernels only (a replicated set keeps the split E-step)") \
    X("VLGP_ESTEP_LANEPT", estep_lanept, TRI, -1, 0, 1, "split E-step: 0 keeps the wave-per-task kernels for ranks <= 14") \
    X("VLGP_ESTEP_NO_SHARED_G", estep_no_shared_g, FLAG, false, 0, 1, "split E-step: per-wave staging of G in the rank <= 16 launches, no lane-per-task launches") \
    X("VLGP_ESTEP_MIX", estep_mix, TRI, -1, 0, 1, "split E-step: 0 launches lane-per-task and wave-per-task latents separately") \
    X("VLGP_ESTEP_LANES", estep_lanes, INT, 0, 1, VLGP_E_LANES, "split E-step: number of stream lanes (default: by set size, one or two)") \
    X("VLGP_LANE_PRIO", lane_prio, INT, 0, 0, 3, "instruction priority of the lane-per-task launches' waves")                \
    X("VLGP_LANE_CLOCK", lane_clock, INT, 0, 0, 2, "phase clock of the lane-per-task launches: 1 factor, 2 mean (vlgp_debug_phase_clock)") \
    X("VLGP_MSTEP_GENERIC", mstep_generic, FLAG, false, 0, 1, "M-step: the loop-based kernels at any size")                    \
    X("VLGP_MSTEP_WG_PER_CU", mstep_wg_per_cu, REAL, 1.0, 0.0, 1e300, "M-step accumulation: workgroups per compute unit")       \
    X("VLGP_NOISE_PASSES", noise_passes, FLAG, false, 0, 1, "M-step: the noise variance by two passes over the rows, not from the moments") \
    X("VLGP_NO_MGRAPH", no_mgraph, FLAG, false, 0, 1, "M-step: enqueue every launch instead of replaying the captured graph") \
    X("VLGP_ICHOL_BLOCK", ichol_block, FLAG, false, 0, 1, "prior factor: lengths <= 64 through the workgroup kernel of the long ones") \
    X("VLGP_NORMS_BLOCKS", norms_blocks, INT, 256, 1, 1024, "norms pass: largest number of workgroups (its partial sums have 1024 slots)") \
    X("VLGP_HSTEP_DENSE", hstep_dense, FLAG, false, 0, 1, "H-step: the dense matrix-pipe round, never the low-rank one")     \
    X("VLGP_HSTEP_GENERIC", hstep_generic, FLAG, false, 0, 1, "H-step: the generic kernels (the reference's omega retry)")     \
    X("VLGP_HSTEP_LOWRANK", hstep_lowrank, FLAG, false, 0, 1, "H-step: the low-rank round whatever the size rule says")        \
    X("VLGP_HSTEP_GENERIC_SEG", hstep_generic_seg, FLAG, false, 0, 1, "H-step: windows 65 ... 128 on the generic kernels")     \
    X("VLGP_HSTEP_FUSE_TABLES", hstep_fuse_tables, FLAG, false, 0, 1, "H-step: every low-rank round workgroup factors its kernel blocks itself (rejected: slower)") \
    X("VLGP_HSTEP_NO_WLM", hstep_no_wlm, FLAG, false, 0, 1, "H-step: the rounds read w row-major, no latent-major copy")       \
    X("VLGP_HSTEP_LR_TOL", hstep_lr_tol, REAL, 1e-12, 0.0, 1e300, "H-step: relative tolerance of the low-rank round's rank prediction") \
    X("VLGP_DEBUG_OCC", debug_occ, FLAG, false, 0, 1, "print occupancy of the fast E-step launch and the H-step's fall-backs on stderr")
#define VLGP_SW_T_FLAG bool
#define VLGP_SW_T_TRI int
#define VLGP_SW_T_INT int
#define VLGP_SW_T_REAL double
struct Switches {
#define X(name, field, kind, def, lo, hi, what) VLGP_SW_T_##kind field = def;
    VLGP_SWITCHES(X)
#undef X
};
void vlgp_read_switches(struct vlgp_ctx* ctx);

// One lane of collectives: an RCCL communicator or the shared-memory test transport (VLGP_COMM_TRANSPORT=shm), neither on
// a single rank, and the stream its all-reduces are enqueued on.
struct HostExchange;
enum { LANE_MAIN = 0, LANE_M = 1 };
struct CommLane {
    void* rccl = nullptr;         // ncclComm_t
    HostExchange* shm = nullptr;
    hipStream_t stream = nullptr; // vlgp_ctx::stream / mstream
    bool open() const { return rccl || shm; }
};

struct ProfSlot {
    int64_t launches = 0;
    double ms = 0.0;
    double units = 0.0;  // work units covered by the timed launches (kernel specific)
};

struct vlgp_ctx {
    int dev = 0;
    DevStream stream;
    int N = 0, L = 0, P = 0, R = 0;
    int n_cu = 256;
    std::vector<uint8_t> gauss;   // host copy
    int n_gauss = 0;
    DevPtr<int> d_gauss;          // (N) int flags
    DevPtr<double> d_a, d_b, d_noise, d_da, d_db;
    bool have_params = false;

    std::map<int, Prior> priors;
    uint64_t prior_epoch = 1;
    DevPtr<const double*> d_prior_base;     // table row -> compact base pointer
    DevPtr<int> d_prior_rl;                 // (rows, L)
    DevPtr<int64_t> d_prior_goff;           // (rows, L)
    int prior_rows = 0;
    // mailbox of the prior kernel: per launch slot the L ranks, then a sequence word (mapped host memory)
    HostPtr<int> h_prior_mb;
    DevPtr<int> d_prior_mb_host;            // device view of h_prior_mb (borrowed)
    DevPtr<int> d_prior_mb;                 // device slots + arrival counter
    unsigned long long prior_seq = 0;
    std::vector<struct Prior*> prior_pending;   // launched, host-side ranks not taken yet (vlgp_prior_collect)
    unsigned long long prior_pending_seq = 0;

    UnitSet sets[VLGP_MAX_SETS];

    // second execution lane: the M-step runs here, concurrently with the H-step
    // rounds on the main stream (they touch disjoint data: a, b vs omega)
    DevStream mstream;
    GrowBuf<double> d_work_m;
    GrowBuf<double> d_mcov;       // vlgp_mstep_cov: first bad row | mu | cov of the call (mstep_cov_layout, call_block.h)
    DevPtr<int> d_fail_m;
    DevEvent ev_fork, ev_m_start, ev_m_done;
    bool m_pending = false;
    // single rank: the M-step's launch sequence (52 launches at Mniter = 25) as an instantiated hipGraph, replayed while
    // its key (buffers, sizes, options) is unchanged: one enqueue instead of ~0.25 ms of host launch calls in front of
    // the H-step's first round
    void* m_graph_exec = nullptr;
    std::vector<double> m_graph_key;

    DevPtr<double> d_ecols;       // E-step per-channel records + wconst (fast kernel), rebuilt per launch
    DevPtr<int> d_fail;           // device failure counter
    DevPtr<unsigned long long> d_clk;     // E-step per-phase cycle counters (debug), 8 slots
    GrowBuf<double> d_work;       // general workspace (M-step partials, H-step, reductions)
    HostGrowBuf<double> h_pinned; // small pinned staging buffer
    // H-step round kernel: device flags/counter and the mapped host mailbox it publishes to
    DevPtr<unsigned> d_hsync;
    HostPtr<double> h_hres;       // 48 results + sequence word
    DevPtr<double> d_hres;        // device view of h_hres (borrowed)
    unsigned h_seq = 0;
    GrowBuf<double> d_hmpart;     // their partial sums by chunks of segments
    bool hprep = false;           // vlgp_hstep_prepare built moments and the w copy for write_epoch hprep_epoch
    DevEvent ev_e_done;           // behind the last launch of the most recent vlgp_estep call (vlgp_estep_wait)
    bool e_done_valid = false;
    uint64_t hprep_epoch = 0, write_epoch = 0;  // write_epoch: bumped by every entry point that may change unit state
    GrowBuf<double> d_hmom;       // (L, T, T) second moments of mu for the quadratic terms
    const UnitSet* hmom_us = nullptr;
    int hmom_T = 0;
    bool hmom_bracket = false;    // inside vlgp_hstep_begin/end: d_hmom stays valid across objective calls
    GrowBuf<double> d_hwlm;       // inside the bracket: w of the set latent-major, (L, rows), for the round kernels
    bool hwlm_valid = false;
    // low-rank H-step round (hstep_lr.h): per (window, dt, tol) the largest omega whose folded kernel blocks have rank <= r
    struct LrThr { int T; double dt, tol; std::vector<double> om; };
    std::vector<LrThr> lr_thr;
    Switches sw;                  // the environment's switches as read at create / reload (VLGP_SWITCHES)
    std::vector<const void*> lds_attr_done;  // kernels whose dynamic-LDS ceiling was raised on this handle's device
    // instruction priority of the round kernels' waves beside the M-step lane: high while the H-step bracket is the longer
    // of the two (durations of the previous EM iteration; hstep.hip, hstep_wave_prio)
    int h_prio = 1;
    double last_h_ms = 0.0, last_m_ms = 0.0;  // 0 = unknown
    double h_t0 = 0.0;
    int last_hstep_path = 0;      // VLGP_PATH_HSTEP_* of the most recent H-step objective call
    double hstat[4] = {0.0, 0.0, 0.0, 0.0};  // vlgp_debug_hstep_stats
    int hplan[VLGP_HSTEP_PLAN_LEN] = {};     // vlgp_debug_hstep_plan: what the most recent objective call launched

    // profiling
    bool prof_on = false;
    ProfSlot prof[VLGP_PROF_KINDS];
    struct PendingProf { int kind; DevEvent a, b; double units; bool done; };
    std::vector<PendingProf> pending;

    // communication (comm.hip): the main lane and the M-step lane's own (collectives of one communicator must not interleave)
    CommLane lanes[2];
    HostExchange* hx = nullptr;   // host-side exchange segment for the H-step round sums (single node)
    int rank = 0, world = 1;

    // second lane of the split E-step (estep_split.hip): half of the unit set runs its sweeps here
    DevStream elane[VLGP_E_LANES - 1];
    DevEvent ev_e_fork, ev_e_join[VLGP_E_LANES - 1];
    int last_estep_path = 0;      // VLGP_PATH_ESTEP_* of the most recent E-step / update_w / update_v launch
    int lds_max = 64 * 1024;      // hipDeviceAttributeMaxSharedMemoryPerBlock (gfx950: 160 KB)

    // Pieces of an EM iteration's tail taken off its critical path (api.hip):
    // (1) the norms of mu, dmu for the stopping rule: one kernel queued behind the E-step, results in mapped host memory
    DevPtr<double> d_xwork;       // 1024 x 2 partial sums | ticket
    HostPtr<double> h_xres;       // mapped: |mu|^2, |dmu|^2, sequence word
    DevPtr<double> d_xres;        // its device view (borrowed)
    unsigned long long x_seq = 0;
    int x_pending = 0;            // 1: queued (sequence x_seq), 2: deferred to vlgp_norms_end (several ranks)
    int x_set = -1;
    // (2) the M-step lane leaves a, b, noise, da, db and its failure count in pinned memory behind its last kernel
    HostPtr<double> h_msnap;      // mapped host memory
    DevPtr<double> d_msnap;       // its device view (borrowed)
    bool msnap_valid = false;
    // (3) vlgp_set_params / vlgp_apply_latent_map stage through their own pinned (and device) buffers, reuse guarded by
    // an event: no stream synchronisation in front of the E-step's first launch
    HostPtr<double> h_stage_par;
    HostPtr<double> h_stage_map;
    DevPtr<double> d_stage_map;
    DevEvent ev_stage_par, ev_stage_map;
    bool stage_par_busy = false, stage_map_busy = false;

    // vlgp_elbo's own device buffer (partials, sums, terms, flags): it never borrows d_work, which a prepared H-step owns
    GrowBuf<double> d_elbo;

    std::string err;
};

// the set that owns this set's y / x / xb rows: the set itself, or the source of its replicas
inline UnitSet& vlgp_rows_owner(vlgp_ctx* ctx, UnitSet& us) { return us.rep.src >= 0 ? ctx->sets[us.rep.src] : us; }

// What vlgp_loglik writes for a set, and how its row pass is launched: `slots` rows of four sums, `n_rate` rates and
// grid.y of the launch.
struct LoglikShape { int64_t slots, n_rate; int grid_y; };
inline LoglikShape vlgp_loglik_shape(const vlgp_ctx* ctx, const UnitSet& us) {
    if (us.is(SET_BY_ROW)) return {(int64_t)us.rep.n * ctx->N, us.rep.rows_src * ctx->N, us.rep.n};
    if (us.is(SET_GROUPS)) return {us.rep.n_pairs, us.rep.rows_src * us.rep.n_pairs, us.rep.n_pairs};
    return {ctx->N, us.rows * ctx->N, 1};
}

// ---- error plumbing ------------------------------------------------------
int vlgp_fail(vlgp_ctx* ctx, int code, const char* fmt, ...);
#define HIPCHK(ctx, call)                                                          \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess)                                                     \
            return vlgp_fail(ctx, VLGP_ERR_HIP, "%s failed: %s (%s:%d)", #call,    \
                             hipGetErrorString(e__), __FILE__, __LINE__);          \
    } while (0)
#define NEED_CTX(ctx) \
    if (!(ctx)) return vlgp_fail(nullptr, VLGP_ERR_ARG, "null handle")
#define CHK(expr)                 \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != VLGP_OK) return rc__; \
    } while (0)

// the device view of a mapped host block: borrowed, it goes with the block
template <class T>
inline int device_view(vlgp_ctx* ctx, DevPtr<T>& d, const HostPtr<T>& h) {
    void* p = nullptr;
    HIPCHK(ctx, hipHostGetDevicePointer(&p, h.get(), 0));
    d.borrow(static_cast<T*>(p));
    return VLGP_OK;
}

int vlgp_ensure_work(vlgp_ctx* ctx, int64_t n_doubles);
int vlgp_ensure_pinned(vlgp_ctx* ctx, int64_t n_doubles);
// dynamic-LDS ceiling of kernel fn raised to `bytes`, once per handle: the attribute is per device, one handle = one device
int vlgp_raise_lds(vlgp_ctx* ctx, const void* fn, int bytes);
int vlgp_allreduce(vlgp_ctx* ctx, int lane, double* d_buf, int64_t n);  // in place, sum, on the lane's stream
int vlgp_hx_allreduce(vlgp_ctx* ctx, double* h_vals, int n);   // host values, n <= 64, rank-order sum; needs ctx->hx
void vlgp_comm_close(vlgp_ctx* ctx);  // both lanes and the host exchange
int vlgp_ensure_work_m(vlgp_ctx* ctx, int64_t n_doubles);
int vlgp_join_m(vlgp_ctx* ctx);  // wait for a pending asynchronous M-step
int vlgp_bind_priors(vlgp_ctx* ctx, UnitSet& us);             // (re)build d_unit_prior
int vlgp_refresh_xb(vlgp_ctx* ctx, UnitSet& us);              // xb = x.b when x is general
UnitSet* vlgp_get_set(vlgp_ctx* ctx, int set, bool must_be_valid);

// How a set-taking entry point opens (api.hip): what it waits for and invalidates, in this order, then the set and its
// admission -- which kinds of set the entry point takes and what it says to the others (SET_ADMISSION, api.hip).
enum : unsigned {
    OPEN_COLLECT = 1,   // host-side ranks of a lazy prior build (vlgp_prior_collect)
    OPEN_STALE = 2,     // unit state changes: the cached H-step moments are stale
    OPEN_JOIN = 4,      // vlgp_join_m: the M-step lane and a queued norms pass, write_epoch bumped
    OPEN_WAIT = 8,      // the same two waits without the bump: the call only reads (what vlgp_hstep_prepare built stays)
    OPEN_PARAMS = 16,   // parameters must be set
    OPEN_DEVICE = 32,   // hipSetDevice
    OPEN_EMPTY = 64,    // the slot may be empty (upload, free)
};
struct Admission { const char* what; unsigned kinds; const char* refusal; };
int open_set(vlgp_ctx* ctx, int set, unsigned how, UnitSet** out, const Admission* a);  // (a null: admit() is the caller's)
int admit(vlgp_ctx* ctx, int set, const UnitSet* us, const Admission& a);
extern const Admission admit_vlgp_loglik, admit_vlgp_predictive, admit_vlgp_calibration, admit_vlgp_elbo, admit_vlgp_forecast, admit_vlgp_marginal,
    admit_vlgp_joint_laplace, admit_vlgp_joint_posterior, admit_vlgp_joint_posterior_moments, admit_vlgp_predictive_cov,
    admit_vlgp_calibration_cov, admit_vlgp_pair_moments, admit_vlgp_pair_moments_cov,
    admit_vlgp_lag_moments;  // the scoring entry points' rows of the table (eval_api.hip)

// profiling brackets (HIP events on ctx->stream)
void vlgp_prof_begin(vlgp_ctx* ctx, int kind, hipStream_t st = nullptr);
void vlgp_prof_end(vlgp_ctx* ctx, int kind, double units = 0.0, hipStream_t st = nullptr);

// ---- kernel launchers (one per translation unit) -------------------------
// mode bits for the E-step kernel
#define EM_FACTOR0 1   // factor I + G'WG from the incoming w before the first sweep
#define EM_MEAN 2      // run mean-update sweeps (n_iter of them)
#define EM_W 4         // recompute w
#define EM_V 8         // update v from the factor
// report != null (vlgp_debug_estep_plan): the same dispatch, every family deciding as it does before a launch and
// writing what it would launch into report[EP_*] instead of touching the device; priors are bound, nothing is launched
int launch_estep(vlgp_ctx* ctx, UnitSet& us, int mode, int n_iter, double dmu_bound, int vb, int* report = nullptr);
// slots of that report (include/vlgp_hip.h documents them); EP_CUT: n_lanes + 1 unit indices, EP_RANK / EP_CLASS: per latent
enum { EP_FAMILY = 0, EP_DECLINE, EP_LT, EP_REC, EP_MAXRA, EP_USE_LANE, EP_MIX, EP_MAXRA_HI, EP_RTOP, EP_LO_SHG, EP_N_LANES,
       EP_CUT, EP_CS = EP_CUT + VLGP_E_LANES + 1, EP_NJ, EP_RP, EP_RA, EP_SMALL, EP_RG, EP_RANK, EP_CLASS = EP_RANK + 16,
       EP_LEN = EP_CLASS + 16 };
#define EP_SAME(name) static_assert(EP_##name == VLGP_EP_##name, "vlgp_debug_estep_plan: slot " #name " is part of the ABI")
EP_SAME(FAMILY); EP_SAME(DECLINE); EP_SAME(LT); EP_SAME(REC); EP_SAME(MAXRA); EP_SAME(USE_LANE); EP_SAME(MIX); EP_SAME(MAXRA_HI);
EP_SAME(RTOP); EP_SAME(LO_SHG); EP_SAME(N_LANES); EP_SAME(CUT); EP_SAME(CS); EP_SAME(NJ); EP_SAME(RP); EP_SAME(RA); EP_SAME(SMALL);
EP_SAME(RG); EP_SAME(RANK); EP_SAME(CLASS);
#undef EP_SAME
static_assert(EP_LEN == VLGP_ESTEP_PLAN_LEN, "vlgp_debug_estep_plan: the report's length is part of the ABI");
// runs entirely on ctx->mstream with the M-step lane's workspace / communicator
int launch_mstep(vlgp_ctx* ctx, UnitSet& us, int n_iter, int use_hessian, double eps, double lr,
                 double da_bound, double db_bound);
int mstep_plan_report(vlgp_ctx* ctx, int64_t rows, int out[12]);  // vlgp_debug_mstep_plan: what launch_mstep would launch
// the M-step under a supplied posterior (vlgp_mstep_cov; mstep_cov.hip): d_mu (rows, L) and d_cov (rows, L (L + 1) / 2),
// pair (l, l'), l' <= l, at l (l + 1) / 2 + l', take the place of the set's mu, v.  One rank, L <= 10, P <= 8, the
// compiled kernels: the caller has checked.  launch_mcov_first_bad_row: *d_first = the first row of (mu | cov) with a
// non-finite value, untouched when there is none.  A masked fit set (vlgp_mstep_cov_masked; no Gaussian channel on the
// handle: checked too) takes the masked PREP and noise passes and mstep_cov_accum_masked.
int launch_mstep_cov(vlgp_ctx* ctx, UnitSet& us, const double* d_mu, const double* d_cov, int n_iter, int use_hessian,
                     double eps, double lr, double da_bound, double db_bound);
int launch_mcov_first_bad_row(vlgp_ctx* ctx, int64_t rows, const double* d_mu, const double* d_cov, unsigned long long* d_first,
                              hipStream_t st);
int launch_hstep(vlgp_ctx* ctx, UnitSet& us, int window, double dt, int n_eval, const int* latent,
                 const double* logp, double* ll, double* dll);
// factor the listed priors (bit-exact ichol_gauss), ranks and compact copies included; returns with pr.rl set
int launch_ichol_all(vlgp_ctx* ctx, const std::vector<Prior*>& prs, const double* omega, const double* sigma,
                     bool in_table, bool lazy = false);
int vlgp_prior_collect(vlgp_ctx* ctx);  // host-side ranks of a lazy launch_ichol_all (call before reading Prior::rl)
int launch_compact_prior(vlgp_ctx* ctx, Prior& pr);  // host-injected d_full -> rl, d_compact
int launch_sample_posterior(vlgp_ctx* ctx, int T, int n, const double* d_mu, const double* d_w, const double* d_G,
                            const double* d_eps, double* d_z, double* d_out);
int launch_npx_probe(vlgp_ctx* ctx, int kind, int64_t n, const double* d_a, const double* d_b, double* d_out);
int launch_xb(vlgp_ctx* ctx, UnitSet& us);
int launch_latent_map(vlgp_ctx* ctx, UnitSet& us, const double* d_map, const double* d_shift);
int launch_snapshot_params(vlgp_ctx* ctx, hipStream_t st, double* d_host);  // a | b | noise | da | db | failure count
int launch_norms(vlgp_ctx* ctx, UnitSet& us, double* d_part, unsigned* d_ticket, double* d_host, unsigned long long seq);
// shared rows of overlapping segments: dir 0 copies first unit's tail -> second unit's head (mu if share_mu, v), dir 1 back,
// for the links [l0, l1); launch_links_map applies the latent map once more to both copies of every shared row
int launch_links_copy(vlgp_ctx* ctx, UnitSet& us, int l0, int l1, int dir);
int launch_links_map(vlgp_ctx* ctx, UnitSet& us, const double* d_map, const double* d_shift);
int hstep_prepare(vlgp_ctx* ctx, UnitSet& us, int T, hipStream_t st);  // moments of mu + w latent-major for the rounds (hstep.hip)
int launch_moments(vlgp_ctx* ctx, UnitSet& us);  // tri(L) gram | sum mu | sum v | sum mu^2 | |dmu|^2 at ctx->d_work
int launch_project(vlgp_ctx* ctx, UnitSet& us, const double* d_proj, const double* d_shift, double* d_part,
                   double* d_out);  // mu = y proj - shift; d_out = column sums of y
int launch_gather(vlgp_ctx* ctx, UnitSet& src, UnitSet& dst, int window);
// plug-in rates and per-channel log-likelihood sums of a set (evaluate.hip): d_rate (vlgp_loglik_shape's n_rate) or null;
// d_sums (slots, 4), written in a fixed order
int launch_loglik(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_rate, double* d_sums);
// d_sums (slots, 4) = the partials d_part (slots, n_blk, 4) of each slot added in workgroup order (evaluate.hip)
int launch_sums_finish(vlgp_ctx* ctx, int slots, int n_blk, const double* d_part, double* d_sums);
// posterior-predictive log density of a set's entries and its per-channel sums (predictive.hip), shaped as launch_loglik:
// d_nodes = z (n_nodes) | lwa (n_nodes), 1 <= n_nodes <= 64; d_rate, d_lpd (vlgp_loglik_shape's n_rate each) or null;
// d_part: (slots, ceil(source rows / 256), 4) doubles of the caller's workspace; d_sums (slots, 4)
int launch_predictive(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, double* d_rate, double* d_lpd,
                      double* d_part, double* d_sums);
// calibration sums of a set's predictive distribution (calibrate.hip), shaped as launch_predictive: W = n_bins + n_levels + 3
// columns per slot in G = ceil(W / 4) groups of four; d_levels (n_levels) on the device; d_cdf (n_rate, 2) = lo | hi or
// null; d_part: (slots, G, ceil(source rows / 256), 4) doubles of the caller's workspace; d_sums (slots, 4 G)
int launch_calibration(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, int n_bins, int n_levels,
                       const double* d_levels, int max_count, double* d_cdf, double* d_part, double* d_sums);
// the two above under a supplied posterior of the linear predictor (vlgp_predictive_cov, vlgp_calibration_cov): d_mu
// (rows of the set, L) and d_cov (rows of the set, L (L + 1) / 2), pair (l, l'), l' <= l, at l (l + 1) / 2 + l', take
// the place of the set's mu, v with vb = 1
int launch_predictive_cov(vlgp_ctx* ctx, UnitSet& us, int n_nodes, const double* d_nodes, const double* d_mu,
                          const double* d_cov, double* d_rate, double* d_lpd, double* d_part, double* d_sums);
int launch_calibration_cov(vlgp_ctx* ctx, UnitSet& us, int n_nodes, const double* d_nodes, const double* d_mu,
                           const double* d_cov, int n_bins, int n_levels, const double* d_levels, int max_count,
                           double* d_cdf, double* d_part, double* d_sums);
// pair moments of a plain or masked set's predictive distribution (pairs.hip): d_resid, d_model (replicas, N, N) under the
// set's own mu, v (d_cov null) or under d_mu, d_cov as the two above take them; d_part: the partials of pair_layout
// (call_block.h) for the source's rows; who: the entry point, for the messages
int launch_pair_moments(vlgp_ctx* ctx, const char* who, UnitSet& us, int vb, const double* d_mu, const double* d_cov,
                        double* d_part, double* d_resid, double* d_model);
// lag moments of a plain or masked set's predictive distribution (lags.hip): lags 0 ... K, rp the largest effective rank
// among the set's priors (bound), o = lag_layout (call_block.h) of the call and the regions it names: d_w, d_c, d_flag (read
// and written only when vb), d_part, and d_resid, d_model, d_count (replicas, K + 1, N)
struct LagLayout;
int launch_lag_moments(vlgp_ctx* ctx, UnitSet& us, int vb, int K, int rp, const LagLayout& o, double* d_w, double* d_c,
                       int* d_flag, double* d_part, double* d_resid, double* d_model, double* d_count);
int launch_scatter(vlgp_ctx* ctx, UnitSet& cut, UnitSet& dst, int window);
// expected log-likelihood sums per channel and KL terms per (unit, latent) of a plain set (elbo.hip); rp: the largest
// effective rank among the set's priors; d_part: (N, ceil(rows / 256), 4) doubles of workspace
int launch_elbo(vlgp_ctx* ctx, UnitSet& us, int vb, int rp, double* d_part, double* d_sums, double* d_row_ell,
                double* d_terms, int* d_flag);
// forward prediction of a plain set (forecast.hip): z = g + w o mu per (row, latent) into d_z (rows, L), then per (unit,
// latent) beta = (I + G'WG)^-1 G'z carried along the extension rows; d_ext_off (M + 1): first extension row of each unit,
// d_gx_off (M): offset of the unit's (L, n_ext, R) block inside d_G_ext; d_terms (M, L, 2), d_flag (M, L)
int launch_forecast(vlgp_ctx* ctx, UnitSet& us, int vb, int rp, double* d_z, const int64_t* d_ext_off,
                    const int64_t* d_gx_off, const double* d_G_ext, double* d_mu_ext, double* d_v_ext, double* d_terms,
                    int* d_flag);
int launch_forecast_z(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_z);  // its row pass alone: z = g + w o mu
// importance weights of a plain set (marginal.hip): kc <= 64 joint draws of every latent path from the weight-space
// posterior N(m, H^-1) built from d_z (launch_forecast_z), d_eps (M, L, R, 64) standard normals, sample contiguous.
// Workspace: d_beta (M, L, R, 64), d_c (M, L, 64), d_part (tiles, 64); tile_rows from marginal_tile_rows(L), d_tile_off
// (M + 1): first row tile of each unit.  Out: d_logw (M, 64), d_parts (M, 64, 2) = {ll, sum_l c}, d_flag (M, L)
int marginal_tile_rows(int L);
int launch_marginal(vlgp_ctx* ctx, UnitSet& us, int rp, int kc, const double* d_z, const double* d_eps, double* d_beta,
                    double* d_c, double* d_part, int tile_rows, const int64_t* d_tile_off, int64_t n_tiles, double* d_logw,
                    double* d_parts, int* d_flag);
int launch_marginal_rows(vlgp_ctx* ctx, UnitSet& us, const char* who, int kc, const double* d_beta, const double* d_c,
                         double* d_part, int tile_rows, const int64_t* d_tile_off, int64_t n_tiles, double* d_logw,
                         double* d_parts);  // its row kernel and finish alone: beta_k and c come from the caller
// joint Laplace posterior of a plain set, or of a masked set of one replica (joint.hip).  JointWork: the call's device block cut into its pieces by
// joint_work_doubles (which returns the doubles needed; W may be null to ask), Dmax the largest stacked dimension of the set.
// launch_joint_init: the mean-field start; launch_joint_round: one row pass, the step decision and, where the step was
// accepted, H, its factor and the next direction, W.n_done counting the finished units; launch_joint_finish: stats (M, 8)
// and mu (rows, L) with v (rows, L) or cov (rows, L (L + 1) / 2), or null; who: the entry point, for the messages;
// launch_joint_draw: kc <= 64 draws into d_beta (M, L, R, 64), their c into d_c (M, L, 64)
struct JointWork {
    const char* who = "vlgp_joint_laplace";
    double* base = nullptr;
    int Dmax = 0;
    size_t state_bytes = 0;
    double *beta = nullptr, *dvec = nullptr, *sd = nullptr, *x = nullptr, *llrow = nullptr, *absrow = nullptr, *g = nullptr;
    double *c = nullptr, *res = nullptr, *cur = nullptr, *H = nullptr, *zw = nullptr;
    int *si = nullptr, *n_done = nullptr;
};
int64_t joint_work_doubles(const vlgp_ctx* ctx, const UnitSet& us, int Dmax, JointWork* W);
int launch_joint_init(vlgp_ctx* ctx, UnitSet& us, int rp, const JointWork& W);
int launch_joint_round(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int max_iter, double tol);
int launch_joint_finish(vlgp_ctx* ctx, UnitSet& us, int rp, const JointWork& W, double* d_stats, double* d_mu, double* d_v,
                        double* d_cov);
int launch_joint_draw(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int kc, const double* d_eps, double* d_beta, double* d_c);
// the window moments of the hyperparameter step, after launch_joint_finish: d_part (M, L, window, window), d_S (L, window,
// window) = the sum over the units of sum over a unit's windows of m m' + G_w (H^-1)_ll G_w'
int launch_joint_window_moments(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int window, double* d_part, double* d_S);
