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
// One lane per row, as pred_rows; a lane walks the counts 0 ... y of its entry, so the lanes of a wave run to the largest
// count among their rows and an entry costs 1 + y masses.  The columns are reduced four at a time through block_sums4: a
// slot's partials are G = ceil(W / 4) groups of (n_blk, 4), which launch_sums_finish adds in workgroup order into
// (slots, 4 G) -- the host copies the first W of a row out.  The columns of a group are computed from lo, hi as they are
// needed, so nothing is indexed dynamically in registers.  No atomics: the same bits on every run.
#include "pred_entry.h"

namespace {

struct CalCols {
    int n_bins, n_levels, groups;  // J, C, G = ceil((J + C + 3) / 4)
    int max_count;
    const double* levels;          // global (C)
};

struct CalEntry {
    double lo, hi, pearson;
    bool skip;
};

// one entry; `live` false (a lane past the rows, an entry its replica does not hold out): nothing is computed
__device__ __forceinline__ CalEntry cal_entry(const RowModel& M, int64_t row, int64_t mrow, int n, int nq, const double* zt,
                                              const double* lt, int max_count, bool live) {
    CalEntry e = {0.0, 0.0, 0.0, false};
    if (!live) return e;
    const double m = row_eta(M, row, mrow, n);
    const double yv = M.y[row * M.N + n];
    double s2 = 0.0;
    if (M.vb)
        for (int l = 0; l < M.L; ++l) {
            const double al = M.a[l * M.N + n];
            s2 = fma(M.v[mrow * M.L + l], al * al, s2);
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
    const double lam = exp(clamp10(row_quad(M, mrow, n, m)));
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

// the G groups of four columns of one entry into the slot's partials (slot, group, n_blk, 4); `turn` counts the calls of
// block_sums4 in this workgroup so that its buffers alternate
__device__ __forceinline__ void cal_sums(const CalEntry& e, bool in, const CalCols& K, const double* lev, int64_t slot,
                                         int n_blk, int* turn, double (*red)[4][4], double* part) {
    for (int g = 0; g < K.groups; ++g) {
        double s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = cal_column(e, 4 * g + j, K, lev);
        block_sums4(s, in, (*turn)++, red, part + ((slot * K.groups + g) * n_blk + blockIdx.x) * 4);
    }
}

struct CalArgs {
    RowModel m;            // y, xb of the set's rows (plain) or the source's (replicated); mu, v of the set
    Nodes q;
    CalCols k;
    int n_blk;
    const int* ch;         // group replicas: left-out channel of each pair, else null
    const int* pair_rep;   // group replicas: replica of each pair
    int n_pairs;
    double* cdf;           // plain (rows, N, 2), group replicas (rows, n_pairs, 2): lo | hi, or null
    double* part;          // (slots, G, n_blk, 4)
};

__global__ void __launch_bounds__(256) cal_rows(CalArgs A) {
    __shared__ double red[2][4][4];
    __shared__ double nodes[2 * PRED_NODES];
    __shared__ double lev[4];
    const RowModel& M = A.m;
    nodes_stage(A.q, nodes);
    if ((int)threadIdx.x < A.k.n_levels) lev[threadIdx.x] = A.k.levels[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;                       // pair (0 for a plain set)
    const int64_t mrow = (int64_t)(A.ch ? A.pair_rep[k] : 0) * M.rows + row;  // row of mu, v in the (replicated) set
    const int n0 = A.ch ? A.ch[k] : 0, n1 = A.ch ? n0 + 1 : M.N;
    int turn = 0;
    for (int n = n0; n < n1; ++n) {
        const CalEntry e = cal_entry(M, row, mrow, n, A.q.n, nodes, nodes + PRED_NODES, A.k.max_count, in);
        if (in && A.cdf) {
            const int64_t at = A.ch ? row * A.n_pairs + k : row * M.N + n;
            A.cdf[2 * at] = e.lo;
            A.cdf[2 * at + 1] = e.hi;
        }
        cal_sums(e, in, A.k, lev, A.ch ? k : n, A.n_blk, &turn, red, A.part);
    }
}

// A masked set: blockIdx.y is the replica, a lane takes a source row and walks the channels in plain order, scoring those
// its replica holds out at that row under that replica's posterior (predictive.hip, pred_rows_masked).  cdf was filled
// with NaN; an entry is written by the one replica that holds it out.
struct CalMaskArgs {
    RowModel m;
    Nodes q;
    CalCols k;
    int n_blk, nw;
    const unsigned long long* mask;  // (n_rep rows, nw)
    double* cdf;                     // (rows, N, 2) or null
    double* part;                    // (n_rep N, G, n_blk, 4)
};

__global__ void __launch_bounds__(256) cal_rows_masked(CalMaskArgs A) {
    __shared__ double red[2][4][4];
    __shared__ double nodes[2 * PRED_NODES];
    __shared__ double lev[4];
    const RowModel& M = A.m;
    nodes_stage(A.q, nodes);
    if ((int)threadIdx.x < A.k.n_levels) lev[threadIdx.x] = A.k.levels[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;
    const int64_t mrow = (int64_t)k * M.rows + row;  // row of mu, v and of the mask in the replicated set
    const unsigned long long* mk = A.mask + mrow * A.nw;
    int turn = 0;
    for (int n = 0; n < M.N; ++n) {
        const bool out = in && ((mk[n >> 6] >> (n & 63)) & 1ull);
        const CalEntry e = cal_entry(M, row, mrow, n, A.q.n, nodes, nodes + PRED_NODES, A.k.max_count, out);
        if (out && A.cdf) {
            A.cdf[2 * (row * M.N + n)] = e.lo;
            A.cdf[2 * (row * M.N + n) + 1] = e.hi;
        }
        cal_sums(e, out, A.k, lev, (int64_t)k * M.N + n, A.n_blk, &turn, red, A.part);
    }
}

}  // namespace

int launch_calibration(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, int n_bins, int n_levels,
                       const double* d_levels, int max_count, double* d_cdf, double* d_part, double* d_sums) {
    const LoglikShape S = vlgp_loglik_shape(ctx, us);
    const RowModel m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    const int n_blk = (int)((m.rows + 255) / 256);
    if (n_nodes < 1 || n_nodes > PRED_NODES)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_calibration: n_nodes = %d outside [1, %d]", n_nodes, PRED_NODES);
    if (n_bins < 1 || n_bins > 32 || n_levels < 0 || n_levels > 4 || max_count < 1 || max_count > 65536)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_calibration: n_bins = %d, n_levels = %d or max_count = %d out of range",
                         n_bins, n_levels, max_count);
    const CalCols K = {n_bins, n_levels, (n_bins + n_levels + 3 + 3) / 4, max_count, d_levels};
    if (m.rows < 1 || n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_calibration on an empty set");
    if (S.grid_y > 65535) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_calibration: at most 65535 replicas or (replica, channel) pairs per set");
    if (S.slots > 0x7fffffffLL / (4 * K.groups)) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_calibration: too many (replica, channel) slots");
    const dim3 grid((unsigned)n_blk, (unsigned)S.grid_y);
    if (us.is(SET_BY_ROW)) {
        CalMaskArgs A;
        A.m = m;
        A.q = {n_nodes, d_nodes};
        A.k = K;
        A.n_blk = n_blk;
        A.nw = us.rep.nw;
        A.mask = us.rep.d_mask;
        A.cdf = d_cdf;
        A.part = d_part;
        hipLaunchKernelGGL(cal_rows_masked, grid, dim3(256), 0, ctx->stream, A);
    } else {
        CalArgs A;
        A.m = m;
        A.q = {n_nodes, d_nodes};
        A.k = K;
        A.n_blk = n_blk;
        A.ch = us.rep.d_ch;  // (null, null, 0 unless the set is group replicas)
        A.pair_rep = us.rep.d_pair;
        A.n_pairs = us.rep.n_pairs;
        A.cdf = d_cdf;
        A.part = d_part;
        hipLaunchKernelGGL(cal_rows, grid, dim3(256), 0, ctx->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    return launch_sums_finish(ctx, (int)S.slots * K.groups, n_blk, d_part, d_sums);
}
