// Kernel argument block shared by the generic (estep.hip) and the fast
// (estep_fast.hip) E-step kernels.
#pragma once
#include "ctx.h"

struct EstepArgs {
    int N, L;
    int mode, n_iter, vb;
    double dmu_bound;
    const int64_t* off;
    const int* unit_prior;
    const double* const* prior_base;
    const int* prior_rl;
    const int64_t* prior_goff;
    const double* y;
    const double* xb;  // (rows, N) or null when x == 1
    double* mu;
    double* v;
    double* w;
    double* dmu;
    const double* a;
    const double* b;
    const double* noise;
    const int* gauss;
    double* scratch;       // long units: 3 * rows * L doubles (ra, ya, u)
    double* lc_global;     // long units whose factors do not fit LDS (else null)
    int64_t lc_stride;     // doubles per unit in lc_global
    int* fail;
    int rg;                // lanes per row in the (T x N) passes (power of two <= 64)
    int lds_T;             // SMALL: row capacity of the LDS tiles
    int lds_gsz, lds_lcsz; // doubles reserved for G tiles / factors in LDS
    int lds_scr;           // fast kernel: doubles of the shared scratch region
    unsigned long long* clk; // optional per-phase cycle counters (thread 0 of every block), or null
    const double* cols_g;    // fast kernel: per-channel records (a_l, a_l^2, b, 1/noise), (N, 2*LT+2), global
    const double* wconst_g;  // fast kernel: Gaussian-channel constant of w per latent (L)
};

// Ranks and LDS demands of the prior factors a set uses (those whose length lies in [Tmin, Tmax]), in ONE scan of the
// prior table.  The kernel families size their LDS regions with different paddings, on purpose (a unified rounding
// would change LDS sizes and with them occupancy); each demand is named for its padding.  All zero without priors.
struct RankSummary {
    int rmax = 0;                    // largest effective rank
    int rlat[VLGP_MAX_L] = {};       // ... of each latent
    const Prior* single = nullptr;   // the one prior of a set whose units all have the same length
    int64_t g_odd = 0;               // generic kernels: G of every latent of one unit, T x (r | 1) each, padded to even
    int64_t lc_odd = 0;              //                  their factors, r x (r | 1) each, padded to even
    int64_t g_even = 0;              // fast kernel: G of every latent of one unit, T x (r rounded up to even) each
    int64_t g_even_lo = 0;           // split E-step: the largest such G of ONE latent among those of rank <= 16 set-wide
};
inline RankSummary estep_rank_summary(const vlgp_ctx* ctx, const UnitSet& us) {
    RankSummary S;
    const int L = ctx->L;
    int64_t glat[VLGP_MAX_L] = {};  // largest T x (r rounded up to even) of each latent
    for (auto& kv : ctx->priors) {
        const Prior& pr = kv.second;
        if (pr.T < us.Tmin || pr.T > us.Tmax) continue;
        if (us.Tmin == us.Tmax) S.single = &pr;
        int64_t g_odd = 0, lc_odd = 0, g_even = 0;
        for (int l = 0; l < L; ++l) {
            const int r = pr.rl[l];
            const int64_t g = (int64_t)pr.T * ((r + 1) & ~1);
            S.rlat[l] = r > S.rlat[l] ? r : S.rlat[l];
            glat[l] = g > glat[l] ? g : glat[l];
            g_odd += (int64_t)pr.T * (r | 1);
            lc_odd += (int64_t)r * (r | 1);
            g_even += g;
        }
        S.g_odd = g_odd > S.g_odd ? g_odd : S.g_odd;
        S.lc_odd = lc_odd > S.lc_odd ? lc_odd : S.lc_odd;
        S.g_even = g_even > S.g_even ? g_even : S.g_even;
    }
    for (int l = 0; l < L; ++l) {
        S.rmax = S.rlat[l] > S.rmax ? S.rlat[l] : S.rmax;
        if (S.rlat[l] <= 16 && glat[l] > S.g_even_lo) S.g_even_lo = glat[l];
    }
    S.g_odd = (S.g_odd + 1) & ~1LL;
    S.lc_odd = (S.lc_odd + 1) & ~1LL;
    return S;
}

// Every launcher below takes `report` (see launch_estep, ctx.h): when set it decides as always, writes what it would launch
// into report[EP_*], sets *handled and returns before its first allocation or launch.
// estep_fast.hip: sets *handled = 1 and launches when the fast kernel applies
// (T <= 64, every effective rank <= 32, L <= 8, LDS fits), else leaves 0.  rs: all zero when the mode needs no prior.
int launch_estep_fast(vlgp_ctx* ctx, UnitSet& us, EstepArgs A, const RankSummary& rs, int* handled, int* report = nullptr);

// estep_long.hip: long units (T > 64) with every wave of the workgroup on the per-latent phases;
// declines (leaves *handled = 0) when rank > 50, L > 10 or the LDS budget does not fit.
int launch_estep_long(vlgp_ctx* ctx, UnitSet& us, EstepArgs A, int* handled, int* report = nullptr);

// estep_split.hip: many window-sized units as a sequence of chip-wide launches (passes over rows, one wave per
// (unit, latent) for the factor and mean phases); declines for small sets, T > 64, rank > 32 or L > 10.
int launch_estep_split(vlgp_ctx* ctx, UnitSet& us, EstepArgs E, const RankSummary& rs, int* handled, int* report = nullptr);
