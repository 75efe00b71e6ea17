// Posterior-predictive scores (vlgp_predictive): the log density of every (row, channel) of a unit set with the likelihood
// integrated over the posterior of its linear predictor, and the per-channel sums in vlgp_loglik's slots.
//
//   m = a_n . mu_t + (b x)_tn,   s2 = (a_n^2) . v_t   (s2 = 0 when vb == 0)
//   Gaussian  lpd  = -1/2 log(2 pi (noise_n + s2)) - (y - m)^2 / (2 (noise_n + s2));   rate = m
//             sums = lpd | y | m | y^2
//   Poisson   rate = trunc_exp(m + s2 / 2), the chain of evaluate.hip (row_quad started from m)
//             s2 < 1e-30:  lpd = y log rate - rate - lgamma(y + 1)          (evaluate.hip's expression)
//             otherwise a Gauss-Hermite rule centred at the mode of g(e) = y e - ex(e) - (e - m)^2 / (2 s2),
//             ex(e) = exp(min(e, 10)):  the start e = min(log y, m + y s2) if y > ex(m) else m lies right of the mode or
//             one bounded step left of it, g' is decreasing and concave, so eight Newton steps descend onto it;
//               h = s2 ex(e) + 1,  tau = sqrt(s2) / sqrt(h),  eta_q = e + tau z_q,  c_q = min(eta_q, 10)
//               t_q = lwa_q + y c_q - exp(c_q) - (eta_q - m)^2 / (2 s2)
//               lpd = -1/2 log h + logsumexp_q t_q - lgamma(y + 1)
//             sums = lpd | y | rate | lgamma(y + 1)
//
// The host passes the node tables z_q = sqrt(2) x_q, lwa_q = log(w_q / sqrt(pi)) + x_q^2 of the n_nodes-point rule; they
// sit in LDS and every lane walks them in order (wave-uniform addresses: broadcast reads).  The log-sum-exp is online -- a
// running maximum, the sum rescaled when the maximum moves -- so a term costs two exponentials and nothing is indexed
// dynamically in registers.  The entries of the three forms of set are walked by row_scores (row_walk.h); block_sums4 and
// launch_sums_finish add in a fixed order: no atomics, the same bits on every run.  vlgp_predictive_cov is the same entry
// with m and s2 from a supplied mean and covariance of the latents (CovMoments, row_walk.h) and vb = 1.
#include "pred_entry.h"  // the node tables in LDS and poisson_lognormal, shared with calibrate.hip

namespace {

// one entry under the moments of `src` (row_walk.h).  A checked source whose m or s2 is not finite: lpd and rate are NaN,
// in the entry's outputs and in its sums; y and lgamma(y + 1) or y^2 stay.
template <class Src, class Emit>
__device__ __forceinline__ void pred_entry(const Src& src, const RowModel& M, const Nodes& q, const NodeTables& t, double* rate,
                                           double* lpd, int64_t row, int64_t mrow, int n, bool live, int64_t at, Emit emit) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        const EntryMoments e = src.moments(M, row, mrow, n);
        if (M.gauss[n]) {
            gauss_sums(e.y, e.m, M.noise[n] + e.s2, s);
        } else {
            poisson_sums_at(e.y, src.rate_arg(M, mrow, n, e), s);
            s[0] = e.s2 < 1e-30 ? poisson_ll(s) : poisson_lognormal(e.y, e.m, e.s2, q.n, t.z, t.lwa) - s[3];
        }
        if (Src::checked && !moments_finite(e)) s[0] = s[2] = NAN;
        if (rate) rate[at] = s[2];
        if (lpd) lpd[at] = s[0];
    }
    emit(s);
}

struct PredScorer {
    Nodes q;
    double* rate;  // plain (rows, N), group replicas (rows, n_pairs), masked (rows, N) filled with NaN beforehand; or null
    double* lpd;   // the same layout, or null
    static constexpr int groups = 1;
    typedef NodeTables Lds;
    __device__ void stage(Lds& t) const { nodes_stage(q, t); }
    template <class Emit>
    __device__ __forceinline__ void entry(const RowModel& M, const Lds& t, int64_t row, int64_t mrow, int n, bool live,
                                          int64_t at, Emit emit) const {
        pred_entry(SetMoments{}, M, q, t, rate, lpd, row, mrow, n, live, at, emit);
    }
};

// vlgp_predictive_cov: the same entry under the caller's mu, cov
struct PredCovScorer {
    Nodes q;
    CovMoments src;
    double* rate;
    double* lpd;
    static constexpr int groups = 1;
    typedef NodeTables Lds;
    __device__ void stage(Lds& t) const { nodes_stage(q, t); }
    template <class Emit>
    __device__ __forceinline__ void entry(const RowModel& M, const Lds& t, int64_t row, int64_t mrow, int n, bool live,
                                          int64_t at, Emit emit) const {
        pred_entry(src, M, q, t, rate, lpd, row, mrow, n, live, at, emit);
    }
};

}  // namespace

int launch_predictive(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, double* d_rate, double* d_lpd,
                      double* d_part, double* d_sums) {
    return launch_row_scores(ctx, "vlgp_predictive", us, vb, PredScorer{{n_nodes, d_nodes}, d_rate, d_lpd}, d_part, d_sums);
}

int launch_predictive_cov(vlgp_ctx* ctx, UnitSet& us, int n_nodes, const double* d_nodes, const double* d_mu,
                          const double* d_cov, double* d_rate, double* d_lpd, double* d_part, double* d_sums) {
    return launch_row_scores(ctx, "vlgp_predictive_cov", us, 1, PredCovScorer{{n_nodes, d_nodes}, {d_mu, d_cov}, d_rate, d_lpd},
                             d_part, d_sums);
}
