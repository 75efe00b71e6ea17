// Calibration of the predictive distribution (vlgp_calibration): for every (row, channel) of a unit set the predictive
// distribution function at the observed value, and per slot of vlgp_loglik the sums of a PIT histogram, of the coverage of
// central intervals and of the Pearson dispersion.  m, s2 and rate are vlgp_predictive's (predictive.hip).
//
//   Poisson   k = y.  p(j) = exp(lpd of the count j) exactly as vlgp_predictive has it: the mode-centred rule of
//             pred_entry.h, or the plug-in Poisson mass when s2 < 1e-30.
//             lo = sum_{j < k} p(j), added in the order j = 0, 1, ...;  hi = lo + p(k);  then both min(., 1)
//             mean = rate = trunc_exp(m + s2 / 2),  var = mean + mean^2 expm1(s2): the clamp enters var through mean only
//             y negative, not an integer, not finite or > max_count: skipped -- lo = hi = NaN, the entry adds 1 to the
//             column `skipped` and nothing else.  The loop over counts runs to min(y, max_count) whatever memory holds.
//   Gaussian  lo = hi = 1/2 erfc(-(y - m) / sqrt(2 (noise_n + s2))),  mean = m,  var = noise_n + s2
//   columns   pit_0 ... pit_{J-1} | covered_0 ... covered_{C-1} | pearson | entries | skipped       (W = J + C + 3)
//             pit_j      hi > lo:  clip((e_{j+1} - lo) / (hi - lo), 0, 1) - clip((e_j - lo) / (hi - lo), 0, 1),  e_j = j / J
//                        hi == lo: 1 in bin min(J - 1, floor(lo J))
//             covered_c  hi >= a and lo < 1 - a,  a = (1 - level_c) / 2
//             pearson    (y - mean)^2 / var
//
// One lane per row (row_scores, row_walk.h); a lane walks the counts 0 ... y of its entry, so the lanes of a wave run to
// the largest count among their rows and an entry costs 1 + y masses.  The columns are reduced four at a time through
// block_sums4: a slot's partials are G = ceil(W / 4) groups of (n_blk, 4), which launch_sums_finish adds in workgroup
// order into (slots, 4 G) -- the host copies the first W of a row out.  The columns of a group are computed from lo, hi
// as they are needed, so nothing is indexed dynamically in registers.  No atomics: the same bits on every run.
// vlgp_calibration_cov is the same entry with m and s2 from a supplied mean and covariance of the latents (CovMoments,
// row_walk.h), vb = 1; an entry whose m or s2 is not finite is skipped like a count that cannot be scored.
#include "pred_entry.h"

namespace {

struct CalCols {
    int n_bins, n_levels;          // J, C
    int max_count;
    const double* levels;          // global (C)
};

struct CalEntry {
    double lo, hi, pearson;
    bool skip;
};

// one entry under the moments of `src` (row_walk.h); a checked source whose m or s2 is not finite: skipped, before anything
// is computed from them
template <class Src>
__device__ __forceinline__ CalEntry cal_entry(const Src& src, const RowModel& M, int64_t row, int64_t mrow, int n, int nq,
                                              const double* zt, const double* lt, int max_count) {
    CalEntry e = {0.0, 0.0, 0.0, false};
    const EntryMoments em = src.moments(M, row, mrow, n);
    const double m = em.m, s2 = em.s2, yv = em.y;
    if (Src::checked && !moments_finite(em)) {
        e.lo = e.hi = NAN;
        e.skip = true;
        return e;
    }
    if (M.gauss[n]) {
        const double nz = M.noise[n] + s2, d = yv - m;
        e.lo = e.hi = 0.5 * erfc(-d / sqrt(2.0 * nz));
        e.pearson = d * d / nz;
        return e;
    }
    // (a NaN fails every comparison, an infinity the second)
    if (!(yv >= 0.0 && yv <= (double)max_count && yv == floor(yv))) {
        e.lo = e.hi = NAN;
        e.skip = true;
        return e;
    }
    const int k = min((int)yv, max_count);
    const double lam = exp(clamp10(src.rate_arg(M, mrow, n, em)));
    const double llam = log(lam);
    double lo = 0.0, pk = 0.0;
#pragma unroll 1
    for (int j = 0; j <= k; ++j) {
        const double yj = (double)j;
        const double lg = lgamma(yj + 1.0);
        double lp;
        if (s2 < 1e-30) lp = yj * llam - lam - lg;
        else lp = poisson_lognormal(yj, m, s2, nq, zt, lt) - lg;
        const double p = exp(lp);
        if (j < k) lo += p;
        else pk = p;
    }
    const double d = yv - lam;
    e.lo = fmin(lo, 1.0);
    e.hi = fmin(lo + pk, 1.0);
    e.pearson = d * d / (lam + lam * lam * expm1(s2));
    return e;
}

__device__ __forceinline__ double clip01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// column c of the entry's row of sums (c >= W: 0); lev: the levels in LDS
__device__ __forceinline__ double cal_column(const CalEntry& e, int c, const CalCols& K, const double* lev) {
    const int J = K.n_bins;
    if (e.skip) return c == J + K.n_levels + 2 ? 1.0 : 0.0;
    if (c < J) {
        if (e.hi > e.lo) {
            const double w = e.hi - e.lo;
            return clip01(((double)(c + 1) / J - e.lo) / w) - clip01(((double)c / J - e.lo) / w);
        }
        return c == min(J - 1, (int)floor(e.lo * J)) ? 1.0 : 0.0;
    }
    c -= J;
    if (c < K.n_levels) {
        const double a = (1.0 - lev[c]) / 2.0;
        return (e.hi >= a && e.lo < 1.0 - a) ? 1.0 : 0.0;
    }
    c -= K.n_levels;
    return c == 0 ? e.pearson : c == 1 ? 1.0 : 0.0;
}

struct CalLds { NodeTables t; double lev[4]; };

// the columns of a group are computed from lo, hi as the group is emitted (of a lane that is not live: from zeros)
template <class Src, class Emit>
__device__ __forceinline__ void cal_scorer_entry(const Src& src, const RowModel& M, const Nodes& q, const CalCols& k, int groups,
                                                 double* cdf, const CalLds& l, int64_t row, int64_t mrow, int n, bool live,
                                                 int64_t at, Emit emit) {
    CalEntry e = {0.0, 0.0, 0.0, false};
    if (live) {
        e = cal_entry(src, M, row, mrow, n, q.n, l.t.z, l.t.lwa, k.max_count);
        if (cdf) {
            cdf[2 * at] = e.lo;
            cdf[2 * at + 1] = e.hi;
        }
    }
    for (int g = 0; g < groups; ++g) {
        double s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = cal_column(e, 4 * g + j, k, l.lev);
        emit(s);
    }
}

struct CalScorer {
    Nodes q;
    CalCols k;
    int groups;    // G = ceil((J + C + 3) / 4)
    double* cdf;   // plain (rows, N, 2), group replicas (rows, n_pairs, 2), masked (rows, N, 2) filled with NaN beforehand:
                   // lo | hi; or null
    typedef CalLds Lds;
    __device__ void stage(Lds& l) const {
        nodes_stage(q, l.t);
        if ((int)threadIdx.x < k.n_levels) l.lev[threadIdx.x] = k.levels[threadIdx.x];
    }
    template <class Emit>
    __device__ __forceinline__ void entry(const RowModel& M, const Lds& l, int64_t row, int64_t mrow, int n, bool live,
                                          int64_t at, Emit emit) const {
        cal_scorer_entry(SetMoments{}, M, q, k, groups, cdf, l, row, mrow, n, live, at, emit);
    }
};

// vlgp_calibration_cov: the same entry under the caller's mu, cov
struct CalCovScorer {
    Nodes q;
    CalCols k;
    int groups;
    double* cdf;
    CovMoments src;
    typedef CalLds Lds;
    __device__ void stage(Lds& l) const {
        nodes_stage(q, l.t);
        if ((int)threadIdx.x < k.n_levels) l.lev[threadIdx.x] = k.levels[threadIdx.x];
    }
    template <class Emit>
    __device__ __forceinline__ void entry(const RowModel& M, const Lds& l, int64_t row, int64_t mrow, int n, bool live,
                                          int64_t at, Emit emit) const {
        cal_scorer_entry(src, M, q, k, groups, cdf, l, row, mrow, n, live, at, emit);
    }
};

}  // namespace

int launch_calibration(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, int n_bins, int n_levels,
                       const double* d_levels, int max_count, double* d_cdf, double* d_part, double* d_sums) {
    const CalCols K = {n_bins, n_levels, max_count, d_levels};
    const CalScorer S = {{n_nodes, d_nodes}, K, (n_bins + n_levels + 3 + 3) / 4, d_cdf};
    return launch_row_scores(ctx, "vlgp_calibration", us, vb, S, d_part, d_sums);
}

int launch_calibration_cov(vlgp_ctx* ctx, UnitSet& us, int n_nodes, const double* d_nodes, const double* d_mu,
                           const double* d_cov, int n_bins, int n_levels, const double* d_levels, int max_count,
                           double* d_cdf, double* d_part, double* d_sums) {
    const CalCols K = {n_bins, n_levels, max_count, d_levels};
    const CalCovScorer S = {{n_nodes, d_nodes}, K, (n_bins + n_levels + 3 + 3) / 4, d_cdf, {d_mu, d_cov}};
    return launch_row_scores(ctx, "vlgp_calibration_cov", us, 1, S, d_part, d_sums);
}
