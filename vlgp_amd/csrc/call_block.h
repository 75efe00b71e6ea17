// The frame of a scoring entry point (eval_api.hip): the layout of the call's one device block, the block
// itself and the copies in and out of it.  The layouts are plain integer arithmetic, so a host program without HIP can
// include this header (tests/call_block_driver.cpp); the block and the copies exist under hipcc only.
#pragma once
#include <stdint.h>
static_assert(sizeof(double) == 8, "offsets and pitches count 8-byte doubles");

// Regions of a block of doubles, handed out front to back: each call returns the region's offset (in doubles) and advances.
struct BlockLayout {
    int64_t at = 0;
    int64_t doubles(int64_t n) { const int64_t o = at; at += n; return o; }
    int64_t ints(int64_t n) { return doubles((n + 1) / 2); }  // two int per double
    int64_t i64(int64_t n) { return doubles(n); }             // (offsets count doubles: 8-byte aligned wherever it starts)
    int64_t need() const { return at; }
};

// ---- the blocks of the calls: integers in, named offsets and `need` out; the regions in the order of the block -------
// (a braced list is evaluated left to right: the initialisers below ARE the order of the regions)
// rate (n_rate, when wanted) | sums (slots, 4); the partials live in vlgp_ctx::d_work
struct LoglikLayout { int64_t rate, sums, need; };
inline LoglikLayout loglik_layout(int64_t slots, int64_t n_rate, bool want_rate) {
    BlockLayout b;
    return {b.doubles(want_rate ? n_rate : 0), b.doubles(4 * slots), b.need()};
}

// nodes (z | lwa, 2 x 64) | rate | lpd (n_rate each, when wanted) | sums (slots, 4) | partials (slots, n_blk, 4)
struct PredictiveLayout { int64_t nodes, rate, lpd, sums, part, need; };
inline PredictiveLayout predictive_layout(int64_t slots, int64_t n_rate, int64_t n_blk, bool want_rate, bool want_lpd) {
    BlockLayout b;
    return {b.doubles(128), b.doubles(want_rate ? n_rate : 0), b.doubles(want_lpd ? n_rate : 0), b.doubles(4 * slots),
            b.doubles(slots * n_blk * 4), b.need()};
}

// nodes (z | lwa, 2 x 64) | levels (4) | cdf (n_rate, 2: lo | hi, when wanted) | sums (slots, 4 G) | partials (slots, G,
// n_blk, 4), G = ceil(W / 4) groups of four for the W = n_bins + n_levels + 3 columns of a slot
struct CalibrationLayout { int64_t nodes, levels, cdf, sums, part, groups, need; };
inline CalibrationLayout calibration_layout(int64_t slots, int64_t n_rate, int64_t n_blk, int64_t n_bins, int64_t n_levels,
                                            bool want_cdf) {
    BlockLayout b;
    const int64_t G = (n_bins + n_levels + 3 + 3) / 4;
    return {b.doubles(128), b.doubles(4), b.doubles(want_cdf ? 2 * n_rate : 0), b.doubles(4 * G * slots),
            b.doubles(slots * G * n_blk * 4), G, b.need()};
}

// The siblings that score under a supplied posterior (vlgp_predictive_cov, vlgp_calibration_cov): the sibling's block, then
// mu (post_rows, L) | cov (post_rows, L (L + 1) / 2) over the rows of the posterior's set
struct MomentsLayout { int64_t mu, cov, need; };
inline MomentsLayout moments_layout(int64_t sibling_need, int64_t post_rows, int64_t L) {
    BlockLayout b;
    b.at = sibling_need;
    return {b.doubles(post_rows * L), b.doubles(post_rows * (L * (L + 1) / 2)), b.need()};
}

// vlgp_pair_moments and its _cov sibling (pairs.hip; the sibling's mu, cov go behind the block: moments_layout): partials
// (n_rep, tile_pairs, n_chunks, 2, 64, 64) | resid | model (n_rep, N, N each), for `rows` rows per replica on n_cu compute
// units.  tiles = ceil(N / 64) channel tiles, tile_pairs = tiles (tiles + 1) / 2 pairs I >= J.  A workgroup takes
// chunk_rows rows of one (tile pair, replica): as many chunks as give every compute unit two workgroups, no more than
// keep the partials (64 KiB per workgroup) within PAIR_PART_DOUBLES, and never fewer than PAIR_MIN_CHUNK rows each.
#define PAIR_MIN_CHUNK 32
#define PAIR_PART_DOUBLES (int64_t(1) << 22)  // 32 MiB
struct PairLayout { int64_t part, resid, model, tiles, tile_pairs, chunk_rows, n_chunks, need; };
inline PairLayout pair_layout(int64_t rows, int64_t N, int64_t n_rep, int64_t n_cu) {
    const int64_t tiles = (N + 63) / 64, tile_pairs = tiles * (tiles + 1) / 2, groups = tile_pairs * n_rep;
    const int64_t want = (2 * n_cu + groups - 1) / groups, cap = PAIR_PART_DOUBLES / (groups * 8192);
    const int64_t most = want < cap ? want : (cap > 1 ? cap : 1);
    const int64_t even = (rows + most - 1) / most, chunk_rows = even > PAIR_MIN_CHUNK ? even : PAIR_MIN_CHUNK;
    const int64_t n_chunks = (rows + chunk_rows - 1) / chunk_rows;
    BlockLayout b;
    return {b.doubles(groups * n_chunks * 8192), b.doubles(n_rep * N * N), b.doubles(n_rep * N * N), tiles, tile_pairs,
            chunk_rows, n_chunks, b.need()};
}
// the LDS of a pair_moments workgroup, in doubles: a of both tiles and u of tile J (L, 64 each) | the row's mu and its v or
// packed cov | d, s of both tiles (128 each) | the diagonal's observation variances (64)
inline int64_t pair_lds_doubles(int64_t L) {
    const int64_t npair = L * (L + 1) / 2;
    return 3 * L * 64 + L + (npair > L ? npair : L) + 128 + 128 + 64;
}

// vlgp_lag_moments (lags.hip), for `rows` rows per replica, post_rows = n_rep rows rows of the posterior's set and its
// `tasks` (unit, latent) pairs, lags 0 ... K, on n_cu compute units: w (post_rows, L) | c (post_rows, K + 1, L) | flags
// (tasks) -- none of the three when vb == 0 -- | partials (n_rep, tiles, n_chunks, 3, K + 1, 64) | resid | model | count
// (n_rep, K + 1, N each).  tiles = ceil(N / 64) channel tiles.  A wave takes chunk_rows rows of one (tile, replica): as
// many chunks as give every compute unit eight waves, no more than keep the partials within LAG_PART_DOUBLES, and never
// fewer than LAG_MIN_CHUNK rows each (a chunk also walks the K rows behind it).
#define LAG_MAX 64
#define LAG_GROUP 8  // lags a lane accumulates in registers per walk over its chunk
#define LAG_MIN_CHUNK 128
#define LAG_PART_DOUBLES (int64_t(1) << 22)  // 32 MiB
#define LAG_C_DOUBLES (int64_t(1) << 29)     // 4 GiB: the most the c workspace may take of the call's block
struct LagLayout { int64_t w, c, flag, part, resid, model, count, tiles, chunk_rows, n_chunks, c_doubles, need; };
inline LagLayout lag_layout(int64_t rows, int64_t N, int64_t L, int64_t n_rep, int64_t tasks, int64_t K, bool vb,
                            int64_t n_cu) {
    const int64_t tiles = (N + 63) / 64, groups = tiles * n_rep, K1 = K + 1, post_rows = n_rep * rows;
    const int64_t want = (8 * n_cu + groups - 1) / groups, cap = LAG_PART_DOUBLES / (groups * 3 * K1 * 64);
    const int64_t most = want < cap ? want : (cap > 1 ? cap : 1);
    const int64_t even = (rows + most - 1) / most, chunk_rows = even > LAG_MIN_CHUNK ? even : LAG_MIN_CHUNK;
    const int64_t n_chunks = (rows + chunk_rows - 1) / chunk_rows, c_doubles = vb ? post_rows * K1 * L : 0;
    BlockLayout b;
    return {b.doubles(vb ? post_rows * L : 0), b.doubles(c_doubles), b.ints(vb ? tasks : 0),
            b.doubles(groups * n_chunks * 3 * K1 * 64), b.doubles(n_rep * K1 * N), b.doubles(n_rep * K1 * N),
            b.doubles(n_rep * K1 * N), tiles, chunk_rows, n_chunks, c_doubles, b.need()};
}
// ... and what the call refuses before anything reaches the device (status -1 VLGP_ERR_ARG, -3 VLGP_ERR_STATE): text is a
// format with one %lld, for arg -- the c workspace is refused by its bytes, never chunked silently
struct LagRefusal { int status; const char* text; long long arg; };
inline LagRefusal lag_refusal(int world, int max_lag, int rp, int64_t c_doubles) {
    if (world > 1) return {-3, "vlgp_lag_moments: more than one rank (%lld)", world};
    if (max_lag < 0 || max_lag > LAG_MAX) return {-1, "vlgp_lag_moments: max_lag = %lld, need 0 <= max_lag <= 64", max_lag};
    if (rp > 64) return {-3, "vlgp_lag_moments: a prior factor has rank %lld, at most 64 are supported", rp};
    if (c_doubles > LAG_C_DOUBLES)
        return {-3, "vlgp_lag_moments: the cross-time covariances need %lld bytes of workspace, at most 4294967296 are taken: "
                    "score fewer rows, replicas or lags per call", (long long)(8 * c_doubles)};
    return {0, nullptr, 0};
}
// the LDS of a lag_task wave, in doubles: H (rp, rs) | u of 64 + K rows (+ EW_CH = 8 of slack) | w (64) | 1 / diag Lc (rp)
inline int64_t lag_task_lds_doubles(int64_t rp, int64_t rs, int64_t K) { return rp * rs + (64 + K) * rs + 8 + 64 + rp; }
// ... and of a lag_moments wave, in bytes: a^2 (L, 64) | the ring of d and s (K + 1, 64 each) | of live (K + 1, 64 int)
inline int64_t lag_moments_lds_bytes(int64_t L, int64_t K) { return 8 * (L * 64 + 2 * (K + 1) * 64) + 4 * (K + 1) * 64; }

// partials (N, n_blk, 4) | sums (N, 4) | terms (tasks, 4) | row_ell (rows, when wanted) | flags (tasks)
struct ElboLayout { int64_t part, sums, terms, rows, flag, need; };
inline ElboLayout elbo_layout(int64_t rows, int64_t N, int64_t tasks, int64_t n_blk, bool want_rows) {
    BlockLayout b;
    return {b.doubles(N * n_blk * 4), b.doubles(4 * N), b.doubles(4 * tasks), b.doubles(want_rows ? rows : 0), b.ints(tasks),
            b.need()};
}

// z (rows, L) | G_ext (g_len) | mu_ext | v_ext (n_out each) | terms (tasks, 2) | ext_off (M + 1), gx_off (M) | flags (tasks)
struct ForecastLayout { int64_t z, g, mu, v, terms, tab, flag, need; };
inline ForecastLayout forecast_layout(int64_t rows, int64_t L, int64_t M, int64_t g_len, int64_t n_out) {
    BlockLayout b;
    return {b.doubles(rows * L), b.doubles(g_len), b.doubles(n_out), b.doubles(n_out), b.doubles(2 * M * L), b.i64(2 * M + 1),
            b.ints(M * L), b.need()};
}

// The sample stage of vlgp_marginal and vlgp_joint_laplace, for 64 draws at a time whatever n_samples is (tasks = M L):
// eps | beta (tasks, R, 64 each) | c (tasks, 64) | tile partials (n_tiles, 64) | log_w (M, 64) | parts (M, 64, 2) |
// tile_off (M + 1).  Without draws only the table is left.
struct SampleLayout { int64_t eps, beta, c, part, lw, parts, tab; };
inline SampleLayout sample_layout(BlockLayout& b, int64_t M, int64_t L, int64_t R, int64_t n_tiles, bool draws) {
    const int64_t k = draws ? 64 : 0;
    return {b.doubles(M * L * R * k), b.doubles(M * L * R * k), b.doubles(M * L * k), b.doubles(n_tiles * k), b.doubles(M * k),
            b.doubles(M * 2 * k), b.i64(M + 1)};
}

// z (rows, L) | the sample stage | flags (tasks)
struct MarginalLayout { int64_t z; SampleLayout s; int64_t flag, need; };
inline MarginalLayout marginal_layout(int64_t rows, int64_t L, int64_t R, int64_t M, int64_t n_tiles) {
    BlockLayout b;
    return {b.doubles(rows * L), sample_layout(b, M, L, R, n_tiles, true), b.ints(M * L), b.need()};
}

// the Newton workspace (`work` doubles: joint_work_doubles) | stats (M, 8) | v (rows, L) | the sample stage, when K > 0
struct JointLayout { int64_t work, stats, v; SampleLayout s; int64_t need; };
inline JointLayout joint_layout(int64_t work, int64_t rows, int64_t L, int64_t R, int64_t M, int64_t n_tiles, int64_t K) {
    BlockLayout b;
    return {b.doubles(work), b.doubles(8 * M), b.doubles(rows * L), sample_layout(b, M, L, R, n_tiles, K > 0), b.need()};
}

// vlgp_joint_posterior: the Newton workspace | stats (M, 8) | cov (rows, L (L + 1) / 2); mu lives in the workspace
struct JointPosteriorLayout { int64_t work, stats, cov, need; };
inline JointPosteriorLayout joint_posterior_layout(int64_t work, int64_t rows, int64_t L, int64_t M) {
    BlockLayout b;
    return {b.doubles(work), b.doubles(8 * M), b.doubles(rows * (L * (L + 1) / 2)), b.need()};
}

// vlgp_joint_posterior_moments (window > 0): vlgp_joint_posterior's block, then the window moments' partials (M, L,
// window, window) | their sum S (L, window, window); window = 0 is vlgp_joint_posterior's block itself
struct JointMomentsLayout { JointPosteriorLayout p; int64_t part, S, need; };
inline JointMomentsLayout joint_moments_layout(int64_t work, int64_t rows, int64_t L, int64_t M, int64_t window) {
    const JointPosteriorLayout p = joint_posterior_layout(work, rows, L, M);
    BlockLayout b;
    b.at = p.need;
    return {p, b.doubles(M * L * window * window), b.doubles(L * window * window), b.need()};
}
// ... and what the call refuses for its window, in this order, before anything reaches the device: the window against the
// compiled tile, the largest effective rank of the set against it, and a set without a unit as long as the window
struct JointMomentsRefusal { int status; const char* text; int arg; };  // (text: a format with one %d, for arg)
inline JointMomentsRefusal joint_moments_refusal(int window, int rp, int64_t n_windows) {
    if (window < 2 || window > 64) return {-1, "vlgp_joint_posterior_moments: window = %d, need 2 <= window <= 64", window};
    if (rp > 64) return {-3, "vlgp_joint_posterior_moments: a prior factor has rank %d, at most 64 are supported", rp};
    if (n_windows < 1) return {-3, "vlgp_joint_posterior_moments: no unit of the set is as long as the window (%d)", window};
    return {0, nullptr, 0};
}
// the number of windows of a unit of T rows: T / window whole ones and one more, ending at the last row, when a rest is left
inline int64_t joint_unit_windows(int64_t T, int64_t window) {
    return T < window ? 0 : T / window + (T % window ? 1 : 0);
}

// vlgp_mstep_cov: the first row with a non-finite moment (one 64-bit integer) | mu (rows, L) | cov (rows, L (L + 1) / 2),
// the handle's own buffer (vlgp_ctx::d_mcov), on the device for all Newton iterations of the call
struct MstepCovLayout { int64_t first, mu, cov, need; };
inline MstepCovLayout mstep_cov_layout(int64_t rows, int64_t L) {
    BlockLayout b;
    return {b.i64(1), b.doubles(rows * L), b.doubles(rows * (L * (L + 1) / 2)), b.need()};
}
// ... and what the call refuses before anything reaches the device: status 0 (VLGP_OK), -1 (VLGP_ERR_ARG, the text names
// the argument) or -3 (VLGP_ERR_STATE, the text says why) -- the limits of the compiled kernels first, then the arguments
struct MstepCovRefusal { int status; const char* text; };
inline MstepCovRefusal mstep_cov_refusal(int L, int P, bool generic_switch, int world, const void* mu, const void* cov,
                                         int n_iter) {
    if (L > 10) return {-3, "vlgp_mstep_cov: more than 10 latents (L > 10): the loop-based M-step kernels take no covariance"};
    if (P > 8) return {-3, "vlgp_mstep_cov: more than 8 regressors (P > 8): the loop-based M-step kernels take no covariance"};
    if (generic_switch) return {-3, "vlgp_mstep_cov: VLGP_MSTEP_GENERIC is set: the loop-based M-step kernels take no covariance"};
    if (world > 1) return {-3, "vlgp_mstep_cov: more than one rank"};
    if (!mu) return {-1, "vlgp_mstep_cov needs mu"};
    if (!cov) return {-1, "vlgp_mstep_cov needs cov"};
    if (n_iter < 1) return {-1, "vlgp_mstep_cov: n_iter must be at least 1"};
    return {0, nullptr};
}
// vlgp_mstep_cov_masked (a masked fit set; the moments' block is mstep_cov_layout): the same order, after the one thing the
// masked kernels cannot do at all -- a Gaussian channel's least squares would need a masked Gram matrix per channel
inline MstepCovRefusal mstep_cov_masked_refusal(int n_gauss, int L, int P, bool generic_switch, int world, const void* mu,
                                                const void* cov, int n_iter) {
    if (n_gauss > 0) return {-3, "vlgp_mstep_cov_masked: the handle has Gaussian channels (their least-squares update needs "
                                 "per-channel masked Gram matrices)"};
    if (L > 10) return {-3, "vlgp_mstep_cov_masked: more than 10 latents (L > 10): the loop-based M-step kernels take no covariance"};
    if (P > 8) return {-3, "vlgp_mstep_cov_masked: more than 8 regressors (P > 8): the loop-based M-step kernels take no covariance"};
    if (generic_switch) return {-3, "vlgp_mstep_cov_masked: VLGP_MSTEP_GENERIC is set: the loop-based M-step kernels take no covariance"};
    if (world > 1) return {-3, "vlgp_mstep_cov_masked: more than one rank"};
    if (!mu) return {-1, "vlgp_mstep_cov_masked needs mu"};
    if (!cov) return {-1, "vlgp_mstep_cov_masked needs cov"};
    if (n_iter < 1) return {-1, "vlgp_mstep_cov_masked: n_iter must be at least 1"};
    return {0, nullptr};
}

#ifdef __HIPCC__
#include "ctx.h"
static_assert(VLGP_ERR_ARG == -1 && VLGP_ERR_STATE == -3, "mstep_cov_refusal spells the status codes out");

// The call's own device block.  Leaving the call, by whichever return, waits for what the call queued on the stream and
// frees the block: early CHK / HIPCHK returns are safe.
struct CallBlock {
    vlgp_ctx* ctx;
    DevPtr<double> d;
    explicit CallBlock(vlgp_ctx* c) : ctx(c) {}
    ~CallBlock() {
        if (d) (void)hipStreamSynchronize(ctx->stream);
    }
    hipError_t alloc(int64_t need) { return d.alloc((size_t)need); }
    double* at(int64_t o) const { return d + o; }
    double* opt(bool want, int64_t o) const { return want ? d + o : nullptr; }
    int* ints(int64_t o) const { return reinterpret_cast<int*>(d + o); }
    int64_t* i64(int64_t o) const { return reinterpret_cast<int64_t*>(d + o); }
};

// Copies on the context's stream that remember the first error: after one, the rest are skipped.
struct Copies {
    vlgp_ctx* ctx;
    hipError_t e = hipSuccess;
    explicit Copies(vlgp_ctx* c) : ctx(c) {}
    void in(void* dev, const void* host, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream);
    }
    void out(void* host, const void* dev, size_t bytes) {  // (an output the caller did not ask for is skipped)
        if (host && e == hipSuccess) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    // `rows` rows of `width` doubles, `dpitch` and `spitch` doubles apart
    void in2d(double* dev, size_t dpitch, const double* host, size_t spitch, size_t width, size_t rows) {
        if (e == hipSuccess) e = hipMemcpy2DAsync(dev, dpitch * 8, host, spitch * 8, width * 8, rows, hipMemcpyHostToDevice, ctx->stream);
    }
    void out2d(double* host, size_t dpitch, const double* dev, size_t spitch, size_t width, size_t rows) {
        if (host && e == hipSuccess)
            e = hipMemcpy2DAsync(host, dpitch * 8, dev, spitch * 8, width * 8, rows, hipMemcpyDeviceToHost, ctx->stream);
    }
    void nan_fill(double* dev, int64_t n) {  // NaN: every byte 0xff
        if (n > 0 && e == hipSuccess) e = hipMemsetAsync(dev, 0xff, sizeof(double) * (size_t)n, ctx->stream);
    }
    // "<who> <what> failed: ..." if a copy did; finish() synchronises first
    int status(const char* who, const char* what) {
        return e == hipSuccess ? VLGP_OK : vlgp_fail(ctx, VLGP_ERR_HIP, "%s %s failed: %s", who, what, hipGetErrorString(e));
    }
    int finish(const char* who, const char* what) {
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        return status(who, what);
    }
};
#endif
