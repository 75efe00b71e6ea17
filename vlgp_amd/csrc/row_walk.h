// What the row scores share (evaluate.hip, predictive.hip, calibrate.hip): the walk of one lane per row over
// the (row, channel) entries of a plain, group-replicated or masked set, its launch, and the per-entry pieces more than
// one scorer uses.  A scorer is a struct passed to the kernel by value:
//
//   struct Lds;                      what it keeps in LDS (may be empty)
//   int groups;                      groups of four sums per slot (may be static)
//   void stage(Lds&) const;          fills Lds, called by every thread before the walk; the walk synchronises
//   void entry(M, lds, row, mrow, n, live, at, emit) const;
//                                    one entry: when live, its per-entry outputs to index `at` of its own arrays; then
//                                    emit(s) once per group, in order, with the group's four sums.  Every thread calls
//                                    emit `groups` times: it holds a barrier.
//
// A lane that is not live -- past the rows, or an entry its replica does not hold out -- computes nothing of its entry,
// and what it emits is not read: it adds 0.0 to every sum.
#pragma once
#include "eval_wave.h"
#include "fast_exp.h"

struct RowWalk {
    RowModel m;            // y, xb of the set's rows (plain) or the source's (replicated); mu, v of the set
    int n_blk;
    const int* ch;         // group replicas: left-out channel of each pair, else null
    const int* pair_rep;   // group replicas: replica of each pair
    int n_pairs;
    const unsigned long long* mask;  // masked set: (n_rep rows, nw)
    int nw;
    double* part;          // (slots, groups, n_blk, 4)
};

//   form            blockIdx.y  mrow                     channels  live             slot     per-entry index
//   plain           0           row                      0..N-1    in               n        row N + n
//   group replicas  pair k      pair_rep[k] rows + row   ch[k]     in               k        row n_pairs + k
//   masked          replica k   k rows + row             0..N-1    in and mask bit  k N + n  row N + n
// The partials of a (slot, group) are one block_sums4 per workgroup; `turn` counts its calls so that its buffers alternate.
template <class Scorer, bool MASKED>
__global__ void __launch_bounds__(256) row_scores(RowWalk A, Scorer S) {
    __shared__ double red[2][4][4];
    __shared__ typename Scorer::Lds lds;
    const RowModel& M = A.m;
    S.stage(lds);
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;
    const bool pairs = !MASKED && A.ch;
    const int64_t mrow = (int64_t)(MASKED ? k : pairs ? A.pair_rep[k] : 0) * M.rows + row;  // row of mu, v and of the mask
    const unsigned long long* mk = MASKED ? A.mask + mrow * A.nw : nullptr;
    const int n0 = pairs ? A.ch[k] : 0, n1 = pairs ? n0 + 1 : M.N;
    int turn = 0;
    for (int n = n0; n < n1; ++n) {
        const bool live = in && (!MASKED || ((mk[n >> 6] >> (n & 63)) & 1ull));
        const int64_t slot = MASKED ? (int64_t)k * M.N + n : pairs ? k : n;
        double* at_part = A.part + (slot * S.groups * A.n_blk + blockIdx.x) * 4;
        S.entry(M, lds, row, mrow, n, live, pairs ? row * A.n_pairs + k : row * M.N + n, [&](const double(&s)[4]) {
            block_sums4(s, live, turn++, red, at_part);
            at_part += (int64_t)A.n_blk * 4;
        });
    }
}

// the row pass of entry point `who` over the set and launch_sums_finish behind it: d_part (slots, groups, n_blk, 4) of
// workspace, d_sums (slots, 4 groups)
template <class Scorer>
static int launch_row_scores(vlgp_ctx* ctx, const char* who, UnitSet& us, int vb, const Scorer& S, double* d_part,
                             double* d_sums) {
    const LoglikShape sh = vlgp_loglik_shape(ctx, us);
    RowWalk A;
    A.m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    A.n_blk = (int)((A.m.rows + 255) / 256);
    A.ch = us.rep.d_ch;  // (null, null, 0 unless the set is group replicas)
    A.pair_rep = us.rep.d_pair;
    A.n_pairs = us.rep.n_pairs;
    A.mask = us.rep.d_mask;
    A.nw = us.rep.nw;
    A.part = d_part;
    if (A.m.rows < 1 || A.n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "%s on an empty set", who);
    if (sh.grid_y > 65535)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: at most 65535 replicas or (replica, channel) pairs per set", who);
    if (sh.slots > 0x7fffffffLL / (4 * S.groups))
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: too many (replica, channel) slots", who);
    const dim3 grid((unsigned)A.n_blk, (unsigned)sh.grid_y);
    if (us.is(SET_BY_ROW)) hipLaunchKernelGGL((row_scores<Scorer, true>), grid, dim3(256), 0, ctx->stream, A, S);
    else hipLaunchKernelGGL((row_scores<Scorer, false>), grid, dim3(256), 0, ctx->stream, A, S);
    HIPCHK(ctx, hipGetLastError());
    return launch_sums_finish(ctx, (int)sh.slots * S.groups, A.n_blk, d_part, d_sums);
}

// ---- per-entry pieces -------------------------------------------------------------------------------------------------
// the posterior of an entry's linear predictor and its observation: m = a_n . mu + (b x), s2 = (a_n^2) . v (0 when
// vb == 0: MAP), y
struct EntryMoments { double m, s2, y; };
__device__ __forceinline__ EntryMoments entry_moments(const RowModel& M, int64_t row, int64_t mrow, int n) {
    EntryMoments e = {row_eta(M, row, mrow, n), 0.0, M.y[row * M.N + n]};
    if (M.vb)
        for (int l = 0; l < M.L; ++l) {
            const double al = M.a[l * M.N + n];
            e.s2 = fma(M.v[mrow * M.L + l], al * al, e.s2);
        }
    return e;
}

// the plug-in sums of an entry.  Gaussian of variance nz about m: ll | y | m | y^2
__device__ __forceinline__ void gauss_sums(double yv, double m, double nz, double (&s)[4]) {
    const double d = yv - m;
    s[0] = -0.5 * log(2.0 * M_PI * nz) - d * d / (2.0 * nz);
    s[1] = yv;
    s[2] = m;
    s[3] = yv * yv;
}

// Poisson at the rate trunc_exp(arg): . | y | rate | lgamma(y + 1); s[0] is the scorer's, poisson_ll(s) the plug-in one
__device__ __forceinline__ void poisson_sums_at(double yv, double arg, double (&s)[4]) {
    s[1] = yv;
    s[2] = exp(clamp10(arg));
    s[3] = lgamma(yv + 1.0);
}
// ... with arg = m + 1/2 (a_n^2) . v, the variance term continuing the chain of m
__device__ __forceinline__ void poisson_sums(const RowModel& M, int64_t mrow, int n, double yv, double m, double (&s)[4]) {
    poisson_sums_at(yv, row_quad(M, mrow, n, m), s);
}
__device__ __forceinline__ double poisson_ll(const double (&s)[4]) { return s[1] * log(s[2]) - s[2] - s[3]; }

// ---- where the moments of an entry come from (predictive.hip, calibrate.hip) -------------------------------------------
// moments(): m, s2, y of an entry; rate_arg(): the argument of the Poisson rate trunc_exp(m + s2 / 2); checked: whether m
// and s2 may be non-finite and the scorer must look (the set's own mu, v are the E-step's and are not looked at).
// SetMoments: the set's mu, v -- entry_moments and the chain of row_quad.
struct SetMoments {
    static constexpr bool checked = false;
    __device__ __forceinline__ EntryMoments moments(const RowModel& M, int64_t row, int64_t mrow, int n) const {
        return entry_moments(M, row, mrow, n);
    }
    __device__ __forceinline__ double rate_arg(const RowModel& M, int64_t mrow, int n, const EntryMoments& e) const {
        return row_quad(M, mrow, n, e.m);
    }
};
// CovMoments: a supplied Gaussian posterior of the latents of every row, mu (rows of the posterior's set, L) and cov
// (the same rows, L (L + 1) / 2), the pair (l, l'), l' <= l, at l (l + 1) / 2 + l'.  m is row_eta's chain with this mu;
//   t_l = sum_l' C[l, l'] a_l'n   a chain of fma from 0 over l' = 0 ... L - 1 (C[l, l'] read at the pair (max, min)),
//   q = sum_l a_ln t_l            a chain of fma from 0 over l = 0 ... L - 1,
// s2 = max(0, q) when q is finite and NaN otherwise; rate_arg = fma(1/2, s2, m).
struct CovMoments {
    const double* mu;
    const double* cov;
    static constexpr bool checked = true;
    __device__ __forceinline__ EntryMoments moments(const RowModel& M, int64_t row, int64_t mrow, int n) const {
        const int L = M.L;
        EntryMoments e = {M.xb ? M.xb[row * M.N + n] : M.b[n], 0.0, M.y[row * M.N + n]};
        for (int l = 0; l < L; ++l) e.m = fma(mu[mrow * L + l], M.a[l * M.N + n], e.m);
        const double* __restrict__ C = cov + mrow * (L * (L + 1) / 2);
        double q = 0.0;
        for (int l = 0; l < L; ++l) {
            double t = 0.0;
            for (int l2 = 0; l2 < L; ++l2) {
                const int hi = max(l, l2), lo = min(l, l2);
                t = fma(C[hi * (hi + 1) / 2 + lo], M.a[l2 * M.N + n], t);
            }
            q = fma(M.a[l * M.N + n], t, q);
        }
        e.s2 = isfinite(q) ? fmax(q, 0.0) : NAN;
        return e;
    }
    __device__ __forceinline__ double rate_arg(const RowModel&, int64_t, int, const EntryMoments& e) const {
        return fma(0.5, e.s2, e.m);
    }
};
__device__ __forceinline__ bool moments_finite(const EntryMoments& e) { return isfinite(e.m) && isfinite(e.s2); }
