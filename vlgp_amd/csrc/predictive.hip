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
// dynamically in registers.  The three forms are evaluate.hip's: pred_rows takes a plain set (one lane per row walking the
// channels) or group replicas (blockIdx.y a (replica, channel) pair), pred_rows_masked a masked set (blockIdx.y the
// replica, the entries its mask holds out).  block_sums4 and launch_sums_finish add in a fixed order: no atomics, the same
// bits on every run.
#include "pred_entry.h"  // the node tables in LDS and poisson_lognormal, shared with calibrate.hip

namespace {

// one entry: the four sums into s, its rate and lpd returned
__device__ __forceinline__ void score_entry(const RowModel& M, int64_t row, int64_t mrow, int n, int nq, const double* zt,
                                             const double* lt, double (&s)[4], double* rate, double* lpd) {
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
        s[0] = -0.5 * log(2.0 * M_PI * nz) - d * d / (2.0 * nz);
        s[2] = m;
        s[3] = yv * yv;
    } else {
        const double lam = exp(clamp10(row_quad(M, mrow, n, m)));
        const double lg = lgamma(yv + 1.0);
        if (s2 < 1e-30) s[0] = yv * log(lam) - lam - lg;
        else s[0] = poisson_lognormal(yv, m, s2, nq, zt, lt) - lg;
        s[2] = lam;
        s[3] = lg;
    }
    s[1] = yv;
    *rate = s[2];
    *lpd = s[0];
}

struct PredArgs {
    RowModel m;            // y, xb of the set's rows (plain) or the source's (replicated); mu, v of the set
    Nodes q;
    int n_blk;
    const int* ch;         // group replicas: left-out channel of each pair, else null
    const int* pair_rep;   // group replicas: replica of each pair
    int n_pairs;
    double* rate;          // plain (rows, N), group replicas (rows, n_pairs), or null
    double* lpd;           // the same layout, or null
    double* part;          // (slots, n_blk, 4)
};

__global__ void __launch_bounds__(256) pred_rows(PredArgs A) {
    __shared__ double red[2][4][4];
    __shared__ double nodes[2 * PRED_NODES];
    const RowModel& M = A.m;
    nodes_stage(A.q, nodes);
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;                       // pair (0 for a plain set)
    const int64_t mrow = (int64_t)(A.ch ? A.pair_rep[k] : 0) * M.rows + row;  // row of mu, v in the (replicated) set
    const int n0 = A.ch ? A.ch[k] : 0, n1 = A.ch ? n0 + 1 : M.N;
    for (int n = n0; n < n1; ++n) {
        double s[4], rate, lpd;
        score_entry(M, row, mrow, n, A.q.n, nodes, nodes + PRED_NODES, s, &rate, &lpd);
        if (in) {
            const int64_t at = A.ch ? row * A.n_pairs + k : row * M.N + n;
            if (A.rate) A.rate[at] = rate;
            if (A.lpd) A.lpd[at] = lpd;
        }
        block_sums4(s, in, n, red, A.part + ((int64_t)(A.ch ? k : n) * A.n_blk + blockIdx.x) * 4);
    }
}

// A masked set: blockIdx.y is the replica, a lane takes a source row and walks the channels in plain order, scoring those
// its replica holds out at that row under that replica's posterior (evaluate.hip, ll_rows_masked).  rate and lpd were
// filled with NaN; an entry is written by the one replica that holds it out.
struct PredMaskArgs {
    RowModel m;
    Nodes q;
    int n_blk, nw;
    const unsigned long long* mask;  // (n_rep rows, nw)
    double* rate;                    // (rows, N) or null
    double* lpd;                     // (rows, N) or null
    double* part;                    // (n_rep N, n_blk, 4)
};

__global__ void __launch_bounds__(256) pred_rows_masked(PredMaskArgs A) {
    __shared__ double red[2][4][4];
    __shared__ double nodes[2 * PRED_NODES];
    const RowModel& M = A.m;
    nodes_stage(A.q, nodes);
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;
    const int64_t mrow = (int64_t)k * M.rows + row;  // row of mu, v and of the mask in the replicated set
    const unsigned long long* mk = A.mask + mrow * A.nw;
    for (int n = 0; n < M.N; ++n) {
        const bool out = in && ((mk[n >> 6] >> (n & 63)) & 1ull);
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (out) {
            double rate, lpd;
            score_entry(M, row, mrow, n, A.q.n, nodes, nodes + PRED_NODES, s, &rate, &lpd);
            if (A.rate) A.rate[row * M.N + n] = rate;
            if (A.lpd) A.lpd[row * M.N + n] = lpd;
        }
        block_sums4(s, out, n, red, A.part + (((int64_t)k * M.N + n) * A.n_blk + blockIdx.x) * 4);
    }
}

}  // namespace

int launch_predictive(vlgp_ctx* ctx, UnitSet& us, int vb, int n_nodes, const double* d_nodes, double* d_rate, double* d_lpd,
                      double* d_part, double* d_sums) {
    const LoglikShape S = vlgp_loglik_shape(ctx, us);
    const RowModel m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    const int n_blk = (int)((m.rows + 255) / 256);
    if (n_nodes < 1 || n_nodes > PRED_NODES)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_predictive: n_nodes = %d outside [1, %d]", n_nodes, PRED_NODES);
    if (m.rows < 1 || n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_predictive on an empty set");
    if (S.grid_y > 65535) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_predictive: at most 65535 replicas or (replica, channel) pairs per set");
    if (S.slots > 0x7fffffffLL / 4) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_predictive: too many (replica, channel) slots");
    const dim3 grid((unsigned)n_blk, (unsigned)S.grid_y);
    if (us.is(SET_BY_ROW)) {
        PredMaskArgs A;
        A.m = m;
        A.q = {n_nodes, d_nodes};
        A.n_blk = n_blk;
        A.nw = us.rep.nw;
        A.mask = us.rep.d_mask;
        A.rate = d_rate;
        A.lpd = d_lpd;
        A.part = d_part;
        hipLaunchKernelGGL(pred_rows_masked, grid, dim3(256), 0, ctx->stream, A);
    } else {
        PredArgs A;
        A.m = m;
        A.q = {n_nodes, d_nodes};
        A.n_blk = n_blk;
        A.ch = us.rep.d_ch;  // (null, null, 0 unless the set is group replicas)
        A.pair_rep = us.rep.d_pair;
        A.n_pairs = us.rep.n_pairs;
        A.rate = d_rate;
        A.lpd = d_lpd;
        A.part = d_part;
        hipLaunchKernelGGL(pred_rows, grid, dim3(256), 0, ctx->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    return launch_sums_finish(ctx, (int)S.slots, n_blk, d_part, d_sums);
}
