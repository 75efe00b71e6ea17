// The read-only scores of a unit set (include/vlgp_hip.h): vlgp_loglik, vlgp_predictive, vlgp_calibration and their _cov
// siblings, vlgp_pair_moments and its, vlgp_lag_moments, vlgp_elbo, vlgp_forecast, vlgp_marginal, vlgp_joint_laplace, vlgp_joint_posterior,
// vlgp_joint_posterior_moments.
// Every one is put together the same way: open the set,
// check the arguments, lay the call's device block out (call_block.h), copy in, launch, copy out.
#include <algorithm>

#include "call_block.h"

// ---- what the row scores (loglik, predictive, calibration) do once their own arguments are sound ----------------------
// admission, no per-entry output from overlapping masks, xb of the rows' owner; then the shapes of vlgp_loglik
struct RowScore { bool by_row; LoglikShape S; int64_t n_blk; };
static int open_row_score(vlgp_ctx* ctx, int set, UnitSet* us, const Admission& a, bool per_entry, const char* outputs,
                          RowScore* r) {
    CHK(admit(ctx, set, us, a));
    r->by_row = us->is(SET_BY_ROW);  // per-entry outputs of such a set: NaN where no replica holds the entry out
    if (r->by_row && per_entry && us->rep.overlap)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: the masks of set %d overlap (an entry is held out by more than one "
                         "replica): no %s, sums only", a.what, set, outputs);
    UnitSet& rows_of = vlgp_rows_owner(ctx, *us);
    if (!rows_of.x_ones) CHK(vlgp_refresh_xb(ctx, rows_of));
    r->S = vlgp_loglik_shape(ctx, *us);
    r->n_blk = (rows_of.rows + 255) / 256;
    return VLGP_OK;
}

extern "C" int vlgp_loglik(vlgp_ctx* ctx, int set, int vb, double* rate, double* sums) {
    UnitSet* us = nullptr;
    // OPEN_JOIN and its epoch bump, not the OPEN_WAIT of a read-only call: launch_loglik's partials live in ctx->d_work,
    // which a prepared H-step may own
    CHK(open_set(ctx, set, OPEN_JOIN | OPEN_PARAMS | OPEN_DEVICE, &us, nullptr));
    if (!sums) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_loglik needs sums");
    RowScore r;
    CHK(open_row_score(ctx, set, us, admit_vlgp_loglik, rate != nullptr, "rate", &r));
    const LoglikLayout o = loglik_layout(r.S.slots, r.S.n_rate, rate != nullptr);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(o.need));
    Copies cp(ctx);
    if (r.by_row && rate) cp.nan_fill(blk.at(o.rate), r.S.n_rate);
    CHK(cp.status("vlgp_loglik:", "filling the rates"));
    CHK(launch_loglik(ctx, *us, vb, blk.opt(rate, o.rate), blk.at(o.sums)));
    cp.out(sums, blk.at(o.sums), sizeof(double) * 4 * (size_t)r.S.slots);
    cp.out(rate, blk.at(o.rate), sizeof(double) * (size_t)r.S.n_rate);
    return cp.finish("vlgp_loglik", "copy-out");
}

// The _cov siblings of vlgp_predictive and vlgp_calibration: the caller's mu (rows, L) and cov (rows, L (L + 1) / 2) over
// the rows of the posterior's set go in behind the sibling's block (moments_layout).  given: the call is such a sibling.
struct Moments { bool given; const double* mu; const double* cov; };
static int need_moments(vlgp_ctx* ctx, const char* who, const Moments& m) {
    if (m.given && !m.mu) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs mu", who);
    if (m.given && !m.cov) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs cov", who);
    return VLGP_OK;
}
static void copy_moments_in(Copies& cp, const CallBlock& blk, const MomentsLayout& o, const Moments& m, int64_t post_rows,
                            int64_t L) {
    cp.in(blk.at(o.mu), m.mu, sizeof(double) * (size_t)(post_rows * L));
    cp.in(blk.at(o.cov), m.cov, sizeof(double) * (size_t)(post_rows * (L * (L + 1) / 2)));
}

// vlgp_loglik's shapes with a second per-entry output; the waits of a read-only call (no epoch bump): the partials are in
// the call's own block
static int predictive_call(vlgp_ctx* ctx, const char* who, const Admission& a, int set, int vb, int n_nodes, const double* z,
                           const double* lwa, const Moments& m, double* rate, double* lpd, double* sums) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_WAIT | OPEN_PARAMS | OPEN_DEVICE, &us, nullptr));
    if (n_nodes < 1 || n_nodes > 64)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: n_nodes = %d, need 1 <= n_nodes <= 64", who, n_nodes);
    if (!z || !lwa || !sums) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs z, lwa and sums", who);
    CHK(need_moments(ctx, who, m));
    RowScore r;
    CHK(open_row_score(ctx, set, us, a, rate || lpd, "rate or lpd", &r));
    if (r.S.slots > 0x7fffffffLL / 4) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: too many (replica, channel) slots", who);
    const PredictiveLayout o = predictive_layout(r.S.slots, r.S.n_rate, r.n_blk, rate != nullptr, lpd != nullptr);
    const MomentsLayout om = moments_layout(o.need, m.given ? us->rows : 0, ctx->L);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(om.need));
    Copies cp(ctx);
    cp.in(blk.at(o.nodes), z, sizeof(double) * (size_t)n_nodes);
    cp.in(blk.at(o.nodes) + n_nodes, lwa, sizeof(double) * (size_t)n_nodes);
    if (m.given) copy_moments_in(cp, blk, om, m, us->rows, ctx->L);
    if (r.by_row) cp.nan_fill(blk.at(o.rate), o.sums - o.rate);  // (rate and lpd lie side by side)
    CHK(cp.status(who, "copy-in"));
    if (m.given)
        CHK(launch_predictive_cov(ctx, *us, n_nodes, blk.at(o.nodes), blk.at(om.mu), blk.at(om.cov), blk.opt(rate, o.rate),
                                  blk.opt(lpd, o.lpd), blk.at(o.part), blk.at(o.sums)));
    else
        CHK(launch_predictive(ctx, *us, vb, n_nodes, blk.at(o.nodes), blk.opt(rate, o.rate), blk.opt(lpd, o.lpd), blk.at(o.part),
                              blk.at(o.sums)));
    cp.out(sums, blk.at(o.sums), sizeof(double) * 4 * (size_t)r.S.slots);
    cp.out(rate, blk.at(o.rate), sizeof(double) * (size_t)r.S.n_rate);
    cp.out(lpd, blk.at(o.lpd), sizeof(double) * (size_t)r.S.n_rate);
    return cp.finish(who, "copy-out");
}

extern "C" int vlgp_predictive(vlgp_ctx* ctx, int set, int vb, int n_nodes, const double* z, const double* lwa,
                               double* rate, double* lpd, double* sums) {
    return predictive_call(ctx, "vlgp_predictive", admit_vlgp_predictive, set, vb, n_nodes, z, lwa, {false, nullptr, nullptr},
                           rate, lpd, sums);
}

extern "C" int vlgp_predictive_cov(vlgp_ctx* ctx, int set, int n_nodes, const double* z, const double* lwa, const double* mu,
                                   const double* cov, double* rate, double* lpd, double* sums) {
    return predictive_call(ctx, "vlgp_predictive_cov", admit_vlgp_predictive_cov, set, 1, n_nodes, z, lwa, {true, mu, cov},
                           rate, lpd, sums);
}

// vlgp_predictive's frame with W columns per slot: the device sums are (slots, 4 G) for the G groups of four that
// launch_sums_finish adds, and the first W of every row go out
static int calibration_call(vlgp_ctx* ctx, const char* who, const Admission& a, int set, int vb, int n_nodes, const double* z,
                            const double* lwa, const Moments& m, int n_bins, int n_levels, const double* levels, int max_count,
                            double* cdf, double* sums) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_WAIT | OPEN_PARAMS | OPEN_DEVICE, &us, nullptr));
    if (n_nodes < 1 || n_nodes > 64) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: n_nodes = %d, need 1 <= n_nodes <= 64", who, n_nodes);
    if (n_bins < 1 || n_bins > 32) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: n_bins = %d, need 1 <= n_bins <= 32", who, n_bins);
    if (n_levels < 0 || n_levels > 4) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: n_levels = %d, need 0 <= n_levels <= 4", who, n_levels);
    if (max_count < 1 || max_count > 65536)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: max_count = %d, need 1 <= max_count <= 65536", who, max_count);
    if (!z || !lwa || !sums) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs z, lwa and sums", who);
    if (n_levels > 0 && !levels) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: n_levels = %d needs levels", who, n_levels);
    CHK(need_moments(ctx, who, m));
    for (int c = 0; c < n_levels; ++c)
        if (!(levels[c] > 0.0 && levels[c] < 1.0))
            return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: levels[%d] = %g, need 0 < level < 1", who, c, levels[c]);
    RowScore r;
    CHK(open_row_score(ctx, set, us, a, cdf != nullptr, "cdf", &r));
    const int W = n_bins + n_levels + 3;
    const CalibrationLayout o = calibration_layout(r.S.slots, r.S.n_rate, r.n_blk, n_bins, n_levels, cdf != nullptr);
    if (r.S.slots > 0x7fffffffLL / (4 * o.groups)) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: too many (replica, channel) slots", who);
    const MomentsLayout om = moments_layout(o.need, m.given ? us->rows : 0, ctx->L);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(om.need));
    Copies cp(ctx);
    cp.in(blk.at(o.nodes), z, sizeof(double) * (size_t)n_nodes);
    cp.in(blk.at(o.nodes) + n_nodes, lwa, sizeof(double) * (size_t)n_nodes);
    if (n_levels) cp.in(blk.at(o.levels), levels, sizeof(double) * (size_t)n_levels);
    if (m.given) copy_moments_in(cp, blk, om, m, us->rows, ctx->L);
    if (r.by_row) cp.nan_fill(blk.at(o.cdf), o.sums - o.cdf);
    CHK(cp.status(who, "copy-in"));
    if (m.given)
        CHK(launch_calibration_cov(ctx, *us, n_nodes, blk.at(o.nodes), blk.at(om.mu), blk.at(om.cov), n_bins, n_levels,
                                   blk.at(o.levels), max_count, blk.opt(cdf, o.cdf), blk.at(o.part), blk.at(o.sums)));
    else
        CHK(launch_calibration(ctx, *us, vb, n_nodes, blk.at(o.nodes), n_bins, n_levels, blk.at(o.levels), max_count,
                               blk.opt(cdf, o.cdf), blk.at(o.part), blk.at(o.sums)));
    cp.out2d(sums, (size_t)W, blk.at(o.sums), (size_t)(4 * o.groups), (size_t)W, (size_t)r.S.slots);
    cp.out(cdf, blk.at(o.cdf), sizeof(double) * 2 * (size_t)r.S.n_rate);
    return cp.finish(who, "copy-out");
}

extern "C" int vlgp_calibration(vlgp_ctx* ctx, int set, int vb, int n_nodes, const double* z, const double* lwa, int n_bins,
                                int n_levels, const double* levels, int max_count, double* cdf, double* sums) {
    return calibration_call(ctx, "vlgp_calibration", admit_vlgp_calibration, set, vb, n_nodes, z, lwa, {false, nullptr, nullptr},
                            n_bins, n_levels, levels, max_count, cdf, sums);
}

extern "C" int vlgp_calibration_cov(vlgp_ctx* ctx, int set, int n_nodes, const double* z, const double* lwa, const double* mu,
                                    const double* cov, int n_bins, int n_levels, const double* levels, int max_count,
                                    double* cdf, double* sums) {
    return calibration_call(ctx, "vlgp_calibration_cov", admit_vlgp_calibration_cov, set, 1, n_nodes, z, lwa, {true, mu, cov},
                            n_bins, n_levels, levels, max_count, cdf, sums);
}

// The pair moments of a plain or masked set (pairs.hip): two (replicas, N, N) matrices, nothing per entry.  Group replicas
// keep one channel group per replica, so no replica holds both channels of a pair: they are told what to make instead.
static int pair_call(vlgp_ctx* ctx, const char* who, const Admission& a, int set, int vb, const Moments& m, double* resid,
                     double* model) {
    UnitSet* us = nullptr;
    CHK(open_set(ctx, set, OPEN_WAIT | OPEN_PARAMS | OPEN_DEVICE, &us, nullptr));
    if (!resid || !model) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs resid and model", who);
    CHK(need_moments(ctx, who, m));
    if (us->is(SET_GROUPS))
        return vlgp_fail(ctx, VLGP_ERR_STATE, "%s: replicate with held_out=: a pair needs both channels in one replica", who);
    CHK(admit(ctx, set, us, a));
    UnitSet& rows_of = vlgp_rows_owner(ctx, *us);
    if (!rows_of.x_ones) CHK(vlgp_refresh_xb(ctx, rows_of));
    if (rows_of.rows < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "%s on an empty set", who);
    const int64_t n_rep = us->is(SET_BY_ROW) ? us->rep.n : 1, nn = n_rep * ctx->N * ctx->N;
    const PairLayout o = pair_layout(rows_of.rows, ctx->N, n_rep, ctx->n_cu);
    const MomentsLayout om = moments_layout(o.need, m.given ? us->rows : 0, ctx->L);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(om.need));
    Copies cp(ctx);
    if (m.given) copy_moments_in(cp, blk, om, m, us->rows, ctx->L);
    CHK(cp.status(who, "copy-in"));
    CHK(launch_pair_moments(ctx, who, *us, vb, blk.opt(m.given, om.mu), blk.opt(m.given, om.cov), blk.at(o.part),
                            blk.at(o.resid), blk.at(o.model)));
    cp.out(resid, blk.at(o.resid), sizeof(double) * (size_t)nn);
    cp.out(model, blk.at(o.model), sizeof(double) * (size_t)nn);
    return cp.finish(who, "copy-out");
}

extern "C" int vlgp_pair_moments(vlgp_ctx* ctx, int set, int vb, double* resid, double* model) {
    return pair_call(ctx, "vlgp_pair_moments", admit_vlgp_pair_moments, set, vb, {false, nullptr, nullptr}, resid, model);
}

extern "C" int vlgp_pair_moments_cov(vlgp_ctx* ctx, int set, const double* mu, const double* cov, double* resid,
                                     double* model) {
    return pair_call(ctx, "vlgp_pair_moments_cov", admit_vlgp_pair_moments_cov, set, 1, {true, mu, cov}, resid, model);
}

// ---- the scores of a posterior (elbo, forecast, marginal, joint Laplace) --------------------------------------------------
// What they do first: a plain set with parameters, xb and its priors bound, nothing pending.  The waits of vlgp_join_m
// without its epoch bump: the calls only read, so what vlgp_hstep_prepare built stays valid.  Then the number of (unit,
// latent) tasks, an int for the launches, and rp, the largest effective rank among the set's lengths: it sizes the LDS of
// the (unit, latent) kernels.  *n_failed starts at 0.
struct Posterior { UnitSet* us = nullptr; int64_t tasks = 0; int rp = 1; };
static int posterior_ready(vlgp_ctx* ctx, const char* what, int* n_failed, Posterior* p);
static int open_posterior(vlgp_ctx* ctx, int set, const Admission& a, int* n_failed, Posterior* p) {
    CHK(open_set(ctx, set, OPEN_COLLECT | OPEN_WAIT | OPEN_PARAMS | OPEN_DEVICE, &p->us, &a));
    return posterior_ready(ctx, a.what, n_failed, p);
}
// ... everything behind the admission (vlgp_lag_moments checks its arguments in between)
static int posterior_ready(vlgp_ctx* ctx, const char* what, int* n_failed, Posterior* p) {
    const UnitSet& us = *p->us;
    UnitSet& rows_of = vlgp_rows_owner(ctx, *p->us);  // (the set itself, or the source of a masked set of one replica)
    if (!rows_of.x_ones) CHK(vlgp_refresh_xb(ctx, rows_of));
    CHK(vlgp_bind_priors(ctx, *p->us));
    p->tasks = (int64_t)us.M * ctx->L;
    if (p->tasks > 0x7fffffffLL) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: too many (unit, latent) pairs", what);
    int T_seen = -1;
    for (int m = 0; m < us.M; ++m) {
        const int T = (int)(us.off[m + 1] - us.off[m]);
        if (T == T_seen) continue;
        T_seen = T;
        const Prior& pr = ctx->priors.find(T)->second;  // (vlgp_bind_priors found every length)
        for (int l = 0; l < ctx->L; ++l) p->rp = std::max(p->rp, pr.rl[l]);
    }
    if (n_failed) *n_failed = 0;
    return VLGP_OK;
}

// the flags of the (unit, latent) tasks, the last of a call's copies out: *n_failed = how many are set
static int count_flags(Copies& cp, const char* who, const int* d_flag, int64_t tasks, int* n_failed) {
    std::vector<int> flag((size_t)tasks);
    cp.out(flag.data(), d_flag, sizeof(int) * (size_t)tasks);
    CHK(cp.finish(who, "copy-out"));
    if (n_failed) *n_failed = (int)(tasks - std::count(flag.begin(), flag.end(), 0));
    return VLGP_OK;
}

extern "C" int vlgp_elbo(vlgp_ctx* ctx, int set, int vb, double* row_sums, double* row_ell, double* kl_terms,
                         int* n_failed) {
    Posterior p;
    CHK(open_posterior(ctx, set, admit_vlgp_elbo, n_failed, &p));
    if (!row_sums || !kl_terms) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_elbo needs row_sums and kl_terms");
    const int64_t rows = p.us->rows;
    const ElboLayout o = elbo_layout(rows, ctx->N, p.tasks, (rows + 255) / 256, row_ell != nullptr);
    // the block is the context's and only grows: a fit under track_elbo calls once per iteration
    HIPCHK(ctx, ctx->d_elbo.ensure(o.need, o.need + o.need / 4, ctx->stream));
    double* d = ctx->d_elbo;
    int* d_flag = reinterpret_cast<int*>(d + o.flag);
    CHK(launch_elbo(ctx, *p.us, vb, p.rp, d + o.part, d + o.sums, row_ell ? d + o.rows : nullptr, d + o.terms, d_flag));
    Copies cp(ctx);
    cp.out(row_sums, d + o.sums, sizeof(double) * 4 * (size_t)ctx->N);
    cp.out(kl_terms, d + o.terms, sizeof(double) * 4 * (size_t)p.tasks);
    cp.out(row_ell, d + o.rows, sizeof(double) * (size_t)rows);
    return count_flags(cp, "vlgp_elbo", d_flag, p.tasks, n_failed);
}

// The lag moments of a plain or masked set (lags.hip): three (replicas, max_lag + 1, N) tables.  The posterior's set is the
// set itself: a masked set of several replicas has units, offsets and bound priors of its own (replica-major), so the
// (unit, latent) tasks cover every replica.  Group replicas score one channel group per replica from pairs the replica
// table lists: they are told what to make instead.
extern "C" int vlgp_lag_moments(vlgp_ctx* ctx, int set, int vb, int max_lag, double* resid, double* model, double* count,
                                int* n_failed) {
    static const char* who = "vlgp_lag_moments";
    Posterior p;
    CHK(open_set(ctx, set, OPEN_COLLECT | OPEN_WAIT | OPEN_PARAMS | OPEN_DEVICE, &p.us, nullptr));
    if (!resid || !model || !count) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs resid, model and count", who);
    LagRefusal no = lag_refusal(ctx->world, max_lag, 0, 0);
    if (no.status) return vlgp_fail(ctx, no.status, no.text, no.arg);
    UnitSet* us = p.us;
    if (us->is(SET_GROUPS))
        return vlgp_fail(ctx, VLGP_ERR_STATE, "%s: replicate with held_out=: the lags of a channel are scored by entry masks", who);
    CHK(admit(ctx, set, us, admit_vlgp_lag_moments));
    CHK(posterior_ready(ctx, who, n_failed, &p));
    UnitSet& rows_of = vlgp_rows_owner(ctx, *us);
    if (rows_of.rows < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "%s on an empty set", who);
    const int64_t n_rep = us->is(SET_BY_ROW) ? us->rep.n : 1, n_out = n_rep * (max_lag + 1) * ctx->N;
    const LagLayout o = lag_layout(rows_of.rows, ctx->N, ctx->L, n_rep, p.tasks, max_lag, vb != 0, ctx->n_cu);
    no = lag_refusal(ctx->world, max_lag, vb ? p.rp : 0, o.c_doubles);
    if (no.status) return vlgp_fail(ctx, no.status, no.text, no.arg);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(o.need));
    Copies cp(ctx);
    CHK(launch_lag_moments(ctx, *us, vb, max_lag, p.rp, o, blk.at(o.w), blk.at(o.c), blk.ints(o.flag), blk.at(o.part),
                           blk.at(o.resid), blk.at(o.model), blk.at(o.count)));
    cp.out(resid, blk.at(o.resid), sizeof(double) * (size_t)n_out);
    cp.out(model, blk.at(o.model), sizeof(double) * (size_t)n_out);
    cp.out(count, blk.at(o.count), sizeof(double) * (size_t)n_out);
    if (!vb) return cp.finish(who, "copy-out");
    return count_flags(cp, who, blk.ints(o.flag), p.tasks, n_failed);
}

extern "C" int vlgp_forecast(vlgp_ctx* ctx, int set, int vb, int n_lengths, const int* lengths, const int* n_ext,
                             const double* G_ext, double* mu_ext, double* v_ext, double* fit_terms, int* n_failed) {
    Posterior p;
    CHK(open_posterior(ctx, set, admit_vlgp_forecast, n_failed, &p));
    UnitSet* us = p.us;
    if (us->is(SET_TILING | SET_COPIED)) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_forecast refuses a cut set (set %d is cut from set %d)", set, us->parent);
    if (n_lengths < 1 || !lengths || !n_ext || !G_ext) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast needs lengths, n_ext and G_ext");
    if (!mu_ext || !v_ext) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast needs mu_ext and v_ext");
    const int L = ctx->L, R = ctx->R, M = us->M;
    std::vector<int64_t> blk_off((size_t)n_lengths + 1, 0);  // offsets of the (L, n_ext[k], R) blocks inside G_ext
    for (int k = 0; k < n_lengths; ++k) {
        if (k > 0 && lengths[k] <= lengths[k - 1])
            return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: lengths must be strictly increasing (lengths[%d] = %d)", k, lengths[k]);
        if (n_ext[k] < 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: n_ext[%d] = %d for length %d, need >= 1", k, n_ext[k], lengths[k]);
        blk_off[(size_t)k + 1] = blk_off[(size_t)k] + (int64_t)L * n_ext[k] * R;
    }
    std::vector<int64_t> tab((size_t)2 * M + 1);  // ext_off (M + 1) | gx_off (M)
    int64_t* ext_off = tab.data();
    int64_t* gx_off = ext_off + M + 1;
    ext_off[0] = 0;
    for (int m = 0; m < M; ++m) {
        const int T = (int)(us->off[m + 1] - us->off[m]);
        const int* at = std::lower_bound(lengths, lengths + n_lengths, T);
        if (at == lengths + n_lengths || *at != T)
            return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: unit %d has length %d, which is not listed", m, T);
        ext_off[m + 1] = ext_off[m] + n_ext[at - lengths];
        gx_off[m] = blk_off[(size_t)(at - lengths)];
    }
    const int64_t g_len = blk_off[(size_t)n_lengths], n_out = ext_off[M] * L;
    const ForecastLayout o = forecast_layout(us->rows, L, M, g_len, n_out);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(o.need));
    int64_t* d_tab = blk.i64(o.tab);
    Copies cp(ctx);
    cp.in(blk.at(o.g), G_ext, sizeof(double) * (size_t)g_len);
    cp.in(d_tab, tab.data(), sizeof(int64_t) * tab.size());
    CHK(cp.status("vlgp_forecast", "copy-in"));
    CHK(launch_forecast(ctx, *us, vb, p.rp, blk.at(o.z), d_tab, d_tab + M + 1, blk.at(o.g), blk.at(o.mu), blk.at(o.v),
                        blk.at(o.terms), blk.ints(o.flag)));
    cp.out(mu_ext, blk.at(o.mu), sizeof(double) * (size_t)n_out);
    cp.out(v_ext, blk.at(o.v), sizeof(double) * (size_t)n_out);
    cp.out(fit_terms, blk.at(o.terms), sizeof(double) * 2 * (size_t)p.tasks);
    return count_flags(cp, "vlgp_forecast", blk.ints(o.flag), p.tasks, n_failed);
}

// ---- the sample stage of vlgp_marginal and vlgp_joint_laplace ----------------------------------------------------------
// first row tile of each unit (M + 1), built once per call
static std::vector<int64_t> tile_table(const UnitSet& us, int tile_rows) {
    std::vector<int64_t> tile_off((size_t)us.M + 1, 0);
    for (int m = 0; m < us.M; ++m)
        tile_off[(size_t)m + 1] = tile_off[(size_t)m] + (us.off[m + 1] - us.off[m] + tile_rows - 1) / tile_rows;
    return tile_off;
}

// K draws, 64 at a time: the chunk of eps (tasks R, K) in, sample contiguous on the device with stride 64; step(kc), the
// caller's launches that turn it into log_w (M, 64) and parts (M, 64, 2); these out into log_w (M, K) and, when wanted,
// parts (M, K, 2).  The copies of a chunk and its kernels are stream-ordered.
template <class Step>
static int sample_stage(Copies& cp, const char* who, const CallBlock& blk, const SampleLayout& s, int64_t tasks_R, int M,
                        int64_t K, const double* eps, double* log_w, double* parts, Step step) {
    for (int64_t k0 = 0; k0 < K; k0 += 64) {
        const int kc = (int)std::min<int64_t>(64, K - k0);
        cp.in2d(blk.at(s.eps), 64, eps + k0, (size_t)K, (size_t)kc, (size_t)tasks_R);
        CHK(cp.status(who, "copy-in"));
        CHK(step(kc));
        cp.out2d(log_w + k0, (size_t)K, blk.at(s.lw), 64, (size_t)kc, (size_t)M);
        cp.out2d(parts ? parts + 2 * k0 : nullptr, (size_t)K * 2, blk.at(s.parts), 128, (size_t)kc * 2, (size_t)M);
        CHK(cp.finish(who, "copy-out"));
    }
    return VLGP_OK;
}

extern "C" int vlgp_marginal(vlgp_ctx* ctx, int set, int vb, int n_samples, const double* eps, double* log_w,
                             double* parts, int* n_failed) {
    static const char* who = "vlgp_marginal";
    Posterior p;
    CHK(open_posterior(ctx, set, admit_vlgp_marginal, n_failed, &p));
    if (n_samples < 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_marginal: n_samples = %d, need >= 1", n_samples);
    if (!eps || !log_w) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_marginal needs eps and log_w");
    UnitSet* us = p.us;
    const int L = ctx->L, R = ctx->R, M = us->M, tile_rows = marginal_tile_rows(L);
    const std::vector<int64_t> tile_off = tile_table(*us, tile_rows);
    const int64_t n_tiles = tile_off[(size_t)M];
    const MarginalLayout o = marginal_layout(us->rows, L, R, M, n_tiles);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(o.need));
    int64_t* d_tab = blk.i64(o.s.tab);
    Copies cp(ctx);
    cp.in(d_tab, tile_off.data(), sizeof(int64_t) * tile_off.size());
    CHK(cp.status(who, "copy-in"));
    CHK(launch_forecast_z(ctx, *us, vb, blk.at(o.z)));
    CHK(sample_stage(cp, who, blk, o.s, p.tasks * R, M, n_samples, eps, log_w, parts, [&](int kc) {
        return launch_marginal(ctx, *us, p.rp, kc, blk.at(o.z), blk.at(o.s.eps), blk.at(o.s.beta), blk.at(o.s.c),
                               blk.at(o.s.part), tile_rows, d_tab, n_tiles, blk.at(o.s.lw), blk.at(o.s.parts), blk.ints(o.flag));
    }));
    return count_flags(cp, who, blk.ints(o.flag), p.tasks, n_failed);
}

// ---- what vlgp_joint_laplace and vlgp_joint_posterior share ----------------------------------------------------------------
// the arguments of the Newton iteration
static int joint_args(vlgp_ctx* ctx, const char* who, int max_iter, double tol) {
    if (max_iter < 1) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: max_iter = %d, need >= 1", who, max_iter);
    if (!(tol > 0.0)) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: tol = %g, need > 0", who, tol);
    return VLGP_OK;
}

// *Dmax: the largest D = sum_l r_l among the units
static int joint_dmax(vlgp_ctx* ctx, const char* who, const UnitSet& us, int* Dmax) {
    *Dmax = 1;
    for (int m = 0; m < us.M; ++m) {  // D = sum_l r_l of the unit's length
        const Prior& pr = ctx->priors.find((int)(us.off[m + 1] - us.off[m]))->second;  // (vlgp_bind_priors found every length)
        int D = 0;
        for (int l = 0; l < ctx->L; ++l) D += pr.rl[l];
        if (D > 512)
            return vlgp_fail(ctx, VLGP_ERR_STATE, "%s: unit %d has D = %d weights, at most 512 are supported", who, m, D);
        *Dmax = std::max(*Dmax, D);
    }
    return VLGP_OK;
}

// the start and the Newton rounds
static int joint_newton(vlgp_ctx* ctx, Copies& cp, const Posterior& p, const JointWork& W, int max_iter, double tol) {
    CHK(launch_joint_init(ctx, *p.us, p.rp, W));
    // every round finishes a unit, factors it (at most max_iter times) or halves its step (at most 30 times per factor)
    for (int64_t round = 0, done = 0; done < p.us->M && round <= 32 * ((int64_t)max_iter + 1); ++round) {
        CHK(launch_joint_round(ctx, *p.us, W, max_iter, tol));
        int nd = 0;
        cp.out(&nd, W.n_done, sizeof(int));
        CHK(cp.finish(W.who, "a Newton round"));
        done = nd;
    }
    return VLGP_OK;
}

// (NaN laplace: the unit failed)
static void count_failed_units(const double* stats, int M, int* n_failed) {
    if (n_failed)
        for (int m = 0; m < M; ++m) *n_failed += stats[8 * (size_t)m] != stats[8 * (size_t)m] ? 1 : 0;
}

extern "C" int vlgp_joint_laplace(vlgp_ctx* ctx, int set, int max_iter, double tol, int n_samples, const double* eps,
                                  double* beta, double* stats, double* mu, double* v, double* log_w, double* parts,
                                  int* n_failed) {
    static const char* who = "vlgp_joint_laplace";
    Posterior p;
    CHK(open_posterior(ctx, set, admit_vlgp_joint_laplace, n_failed, &p));
    CHK(joint_args(ctx, who, max_iter, tol));
    if (n_samples < 0) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_joint_laplace: n_samples = %d, need >= 0", n_samples);
    if (!stats) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_joint_laplace needs stats");
    if (n_samples > 0 && (!eps || !log_w)) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_joint_laplace: n_samples > 0 needs eps and log_w");
    UnitSet* us = p.us;
    const int L = ctx->L, R = ctx->R, M = us->M, tile_rows = marginal_tile_rows(L);
    const int64_t K = n_samples, rows = us->rows;
    int Dmax = 1;
    CHK(joint_dmax(ctx, who, *us, &Dmax));
    const std::vector<int64_t> tile_off = tile_table(*us, tile_rows);
    const int64_t n_tiles = tile_off[(size_t)M];
    const JointLayout o = joint_layout(joint_work_doubles(ctx, *us, Dmax, nullptr), rows, L, R, M, n_tiles, K);
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(o.need));
    JointWork W;
    W.base = blk.at(o.work);
    (void)joint_work_doubles(ctx, *us, Dmax, &W);
    int64_t* d_tab = blk.i64(o.s.tab);
    Copies cp(ctx);
    CHK(joint_newton(ctx, cp, p, W, max_iter, tol));
    const bool path = mu || v;
    CHK(launch_joint_finish(ctx, *us, p.rp, W, blk.at(o.stats), path ? W.g : nullptr, blk.opt(path, o.v), nullptr));
    cp.out(stats, blk.at(o.stats), sizeof(double) * 8 * (size_t)M);
    cp.out(beta, W.beta, sizeof(double) * (size_t)(p.tasks * R));
    cp.out(mu, W.g, sizeof(double) * (size_t)(rows * L));
    cp.out(v, blk.at(o.v), sizeof(double) * (size_t)(rows * L));
    if (K) cp.in(d_tab, tile_off.data(), sizeof(int64_t) * tile_off.size());
    CHK(cp.finish(who, "copy-out"));
    count_failed_units(stats, M, n_failed);
    return sample_stage(cp, who, blk, o.s, p.tasks * R, M, K, eps, log_w, parts, [&](int kc) {
        CHK(launch_joint_draw(ctx, *us, W, kc, blk.at(o.s.eps), blk.at(o.s.beta), blk.at(o.s.c)));
        return launch_marginal_rows(ctx, *us, who, kc, blk.at(o.s.beta), blk.at(o.s.c), blk.at(o.s.part), tile_rows, d_tab,
                                    n_tiles, blk.at(o.s.lw), blk.at(o.s.parts));
    });
}

// vlgp_joint_laplace's mode without draws, on a plain set or a masked set of one replica, with the covariance of every row;
// window > 0 (vlgp_joint_posterior_moments): also the window moments S (L, window, window) and the number of windows, from
// the factor while it is still in the call's block
static int joint_posterior_call(vlgp_ctx* ctx, const char* who, const Admission& a, int set, int max_iter, double tol,
                                double* beta, double* stats, double* mu, double* cov, int* n_failed, int window, double* S,
                                int64_t* n_windows) {
    Posterior p;
    CHK(open_posterior(ctx, set, a, n_failed, &p));
    UnitSet* us = p.us;
    int Dmax = 1;
    CHK(joint_args(ctx, who, max_iter, tol));
    if (!stats) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs stats", who);
    const bool moments = &a == &admit_vlgp_joint_posterior_moments;
    if (moments) {
        if (!S || !n_windows) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s needs S and n_windows", who);
        int64_t nw = 0;
        for (int m = 0; m < us->M && window > 0; ++m) nw += joint_unit_windows(us->off[m + 1] - us->off[m], window);
        const JointMomentsRefusal no = joint_moments_refusal(window, p.rp, nw);
        if (no.status) return vlgp_fail(ctx, no.status, no.text, no.arg);
        *n_windows = nw;
    }
    CHK(joint_dmax(ctx, who, *us, &Dmax));
    const int L = ctx->L, M = us->M;
    const int64_t rows = us->rows, npair = (int64_t)L * (L + 1) / 2;
    const JointMomentsLayout om = joint_moments_layout(joint_work_doubles(ctx, *us, Dmax, nullptr), rows, L, M, window);
    const JointPosteriorLayout& o = om.p;
    CallBlock blk(ctx);
    HIPCHK(ctx, blk.alloc(om.need));
    JointWork W;
    W.who = who;
    W.base = blk.at(o.work);
    (void)joint_work_doubles(ctx, *us, Dmax, &W);
    Copies cp(ctx);
    CHK(joint_newton(ctx, cp, p, W, max_iter, tol));
    const bool path = mu || cov;
    CHK(launch_joint_finish(ctx, *us, p.rp, W, blk.at(o.stats), path ? W.g : nullptr, nullptr, blk.opt(path, o.cov)));
    if (moments) CHK(launch_joint_window_moments(ctx, *us, W, window, blk.at(om.part), blk.at(om.S)));
    cp.out(stats, blk.at(o.stats), sizeof(double) * 8 * (size_t)M);
    cp.out(beta, W.beta, sizeof(double) * (size_t)(p.tasks * ctx->R));
    cp.out(mu, W.g, sizeof(double) * (size_t)(rows * L));
    cp.out(cov, blk.at(o.cov), sizeof(double) * (size_t)(rows * npair));
    if (moments) cp.out(S, blk.at(om.S), sizeof(double) * (size_t)L * window * window);
    CHK(cp.finish(who, "copy-out"));
    count_failed_units(stats, M, n_failed);
    return VLGP_OK;
}

extern "C" int vlgp_joint_posterior(vlgp_ctx* ctx, int set, int max_iter, double tol, double* beta, double* stats, double* mu,
                                    double* cov, int* n_failed) {
    return joint_posterior_call(ctx, "vlgp_joint_posterior", admit_vlgp_joint_posterior, set, max_iter, tol, beta, stats, mu,
                                cov, n_failed, 0, nullptr, nullptr);
}

extern "C" int vlgp_joint_posterior_moments(vlgp_ctx* ctx, int set, int max_iter, double tol, double* beta, double* stats,
                                            double* mu, double* cov, int* n_failed, int window, double* S,
                                            int64_t* n_windows) {
    return joint_posterior_call(ctx, "vlgp_joint_posterior_moments", admit_vlgp_joint_posterior_moments, set, max_iter, tol,
                                beta, stats, mu, cov, n_failed, window, S, n_windows);
}
