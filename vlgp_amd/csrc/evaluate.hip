// Held-out evaluation (vlgp_loglik): plug-in rate and log-likelihood of every (row, channel) of a unit set, and their
// per-channel sums.
//
//   Poisson   rate = trunc_exp(a_n . mu_t + (b x)_tn + 1/2 (a_n^2) . v_t)   (v taken as 0 when vb == 0: MAP)
//             ll   = y log rate - rate - lgamma(y + 1)
//             sums = ll | y | rate | lgamma(y + 1)
//   Gaussian  eta  = a_n . mu_t + (b x)_tn
//             ll   = -1/2 log(2 pi noise_n) - (y - eta)^2 / (2 noise_n)
//             sums = ll | y | eta | y^2
//
// ll_rows: one lane per row.  A plain set walks all N channels of the row in plain channel order (0 ... N-1); a
// replicated set (vlgp_replicate_groups) takes blockIdx.y as a (replica, left-out channel) pair, in the order the
// caller listed the channels, and evaluates that channel under that replica's posterior on the source rows.  The
// variance term continues the chain of eta (row_quad started from eta): elbo_rows and forecast_rows add theirs afterwards
// and differ from this in the last bit.  The four sums of each (channel, workgroup) become a partial per workgroup
// (block_sums4, eval_wave.h); ll_finish, which vlgp_elbo shares, adds the partials of a slot in workgroup order.
#include "eval_wave.h"
#include "fast_exp.h"

namespace {

struct LlArgs {
    RowModel m;            // y, xb of the set's rows (plain) or the source's (replicated); mu, v of the set
    int n_blk;
    const int* ch;         // replicated set: left-out channel of each pair, else null
    const int* pair_rep;   // replicated set: replica of each pair
    int n_pairs;
    double* rate;          // plain (rows, N), replicated (rows, n_pairs), or null
    double* part;          // (slots, n_blk, 4)
};

__global__ void __launch_bounds__(256) ll_rows(LlArgs A) {
    __shared__ double red[2][4][4];
    const RowModel& M = A.m;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;                       // pair (0 for a plain set)
    const int64_t mrow = (int64_t)(A.ch ? A.pair_rep[k] : 0) * M.rows + row;  // row of mu, v in the (replicated) set
    const int n0 = A.ch ? A.ch[k] : 0, n1 = A.ch ? n0 + 1 : M.N;
    for (int n = n0; n < n1; ++n) {
        double eta = row_eta(M, row, mrow, n);
        const double yv = M.y[row * M.N + n];
        double s[4];
        if (M.gauss[n]) {
            const double nz = M.noise[n], d = yv - eta;
            s[0] = -0.5 * log(2.0 * M_PI * nz) - d * d / (2.0 * nz);
            s[2] = eta;
            s[3] = yv * yv;
            if (A.rate && in) A.rate[A.ch ? row * A.n_pairs + k : row * M.N + n] = eta;
        } else {
            eta = row_quad(M, mrow, n, eta);
            const double lam = exp(clamp10(eta));
            const double lg = lgamma(yv + 1.0);
            s[0] = yv * log(lam) - lam - lg;
            s[2] = lam;
            s[3] = lg;
            if (A.rate && in) A.rate[A.ch ? row * A.n_pairs + k : row * M.N + n] = lam;
        }
        s[1] = yv;
        block_sums4(s, in, n, red, A.part + ((int64_t)(A.ch ? k : n) * A.n_blk + blockIdx.x) * 4);
    }
}

// A masked set (vlgp_replicate_masked): blockIdx.y is the replica, a lane takes a source row and walks the channels in
// plain order, evaluating those its replica holds out at that row under that replica's posterior.  Slot (k, n) sums over
// exactly the rows where replica k holds (row, n) out -- the other lanes add zeros, in the same fixed order -- and
// rate[row, n] is written by the replica that holds the entry out (the host has checked that there is at most one).
struct LlMaskArgs {
    RowModel m;
    int n_blk, nw;
    const unsigned long long* mask;  // (n_rep rows, nw)
    double* rate;                    // (rows, N), filled with NaN beforehand, or null
    double* part;                    // (n_rep N, n_blk, 4)
};

__global__ void __launch_bounds__(256) ll_rows_masked(LlMaskArgs A) {
    __shared__ double red[2][4][4];
    const RowModel& M = A.m;
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
            double eta = row_eta(M, row, mrow, n);
            const double yv = M.y[row * M.N + n];
            if (M.gauss[n]) {
                const double nz = M.noise[n], d = yv - eta;
                s[0] = -0.5 * log(2.0 * M_PI * nz) - d * d / (2.0 * nz);
                s[2] = eta;
                s[3] = yv * yv;
                if (A.rate) A.rate[row * M.N + n] = eta;
            } else {
                eta = row_quad(M, mrow, n, eta);
                const double lam = exp(clamp10(eta));
                const double lg = lgamma(yv + 1.0);
                s[0] = yv * log(lam) - lam - lg;
                s[2] = lam;
                s[3] = lg;
                if (A.rate) A.rate[row * M.N + n] = lam;
            }
            s[1] = yv;
        }
        block_sums4(s, out, n, red, A.part + (((int64_t)k * M.N + n) * A.n_blk + blockIdx.x) * 4);
    }
}

// sums[slot][j] = the slot's partials added in workgroup order
__global__ void __launch_bounds__(256) ll_finish(int slots, int n_blk, const double* __restrict__ part,
                                                 double* __restrict__ sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots * 4) return;
    const int slot = i >> 2, j = i & 3;
    double t = 0.0;
    for (int b = 0; b < n_blk; ++b) t += part[((int64_t)slot * n_blk + b) * 4 + j];
    sums[i] = t;
}

}  // namespace

int launch_sums_finish(vlgp_ctx* ctx, int slots, int n_blk, const double* d_part, double* d_sums) {
    hipLaunchKernelGGL(ll_finish, dim3((unsigned)((slots * 4 + 255) / 256)), dim3(256), 0, ctx->stream, slots, n_blk, d_part,
                       d_sums);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

static int launch_loglik_masked(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_rate, double* d_sums) {
    LlMaskArgs A;
    const LoglikShape S = vlgp_loglik_shape(ctx, us);
    A.m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    A.n_blk = (int)((A.m.rows + 255) / 256);
    A.nw = us.rep.nw;
    A.mask = us.rep.d_mask;
    A.rate = d_rate;
    if (A.m.rows < 1 || A.n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_loglik on an empty set");
    if (S.grid_y > 65535) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s", S.limit);
    if (S.slots > 0x7fffffffLL / 4) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_loglik: too many (replica, channel) slots");
    CHK(vlgp_ensure_work(ctx, S.slots * A.n_blk * 4 + 8));
    A.part = ctx->d_work;
    hipLaunchKernelGGL(ll_rows_masked, dim3((unsigned)A.n_blk, (unsigned)S.grid_y), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return launch_sums_finish(ctx, (int)S.slots, A.n_blk, ctx->d_work, d_sums);
}

int launch_loglik(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_rate, double* d_sums) {
    if (us.is(SET_BY_ROW)) return launch_loglik_masked(ctx, us, vb, d_rate, d_sums);
    const LoglikShape S = vlgp_loglik_shape(ctx, us);
    LlArgs A;
    A.m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    A.n_blk = (int)((A.m.rows + 255) / 256);
    A.ch = us.rep.d_ch;  // (null, null, 0 unless the set is group replicas)
    A.pair_rep = us.rep.d_pair;
    A.n_pairs = us.rep.n_pairs;
    A.rate = d_rate;
    if (A.m.rows < 1 || A.n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_loglik on an empty set");
    if (S.grid_y > 65535) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s", S.limit);
    CHK(vlgp_ensure_work(ctx, S.slots * A.n_blk * 4 + 8));
    A.part = ctx->d_work;
    hipLaunchKernelGGL(ll_rows, dim3((unsigned)A.n_blk, (unsigned)S.grid_y), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return launch_sums_finish(ctx, (int)S.slots, A.n_blk, ctx->d_work, d_sums);
}
