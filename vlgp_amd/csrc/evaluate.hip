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
// The entries of a plain, group-replicated or masked set are walked by row_scores (row_walk.h), which also turns the four
// sums of each (slot, workgroup) into a partial; ll_finish, which vlgp_elbo shares, adds the partials of a slot in
// workgroup order.  The variance term continues the chain of eta (row_quad started from eta): elbo_rows and forecast_rows
// add theirs afterwards and differ from this in the last bit.
#include "row_walk.h"

namespace {

struct LoglikScorer {
    double* rate;  // plain (rows, N), group replicas (rows, n_pairs), masked (rows, N) filled with NaN beforehand; or null
    static constexpr int groups = 1;
    struct Lds {};
    __device__ void stage(Lds&) const {}
    template <class Emit>
    __device__ __forceinline__ void entry(const RowModel& M, const Lds&, int64_t row, int64_t mrow, int n, bool live,
                                          int64_t at, Emit emit) const {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            const double eta = row_eta(M, row, mrow, n);
            const double yv = M.y[row * M.N + n];
            if (M.gauss[n]) {
                gauss_sums(yv, eta, M.noise[n], s);
            } else {
                poisson_sums(M, mrow, n, yv, eta, s);
                s[0] = poisson_ll(s);
            }
            if (rate) rate[at] = s[2];
        }
        emit(s);
    }
};

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

// the partials live in ctx->d_work, which is why vlgp_loglik opens with the epoch bump (eval_api.hip)
int launch_loglik(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_rate, double* d_sums) {
    const int64_t n_blk = (vlgp_rows_owner(ctx, us).rows + 255) / 256;
    CHK(vlgp_ensure_work(ctx, vlgp_loglik_shape(ctx, us).slots * n_blk * 4 + 8));
    return launch_row_scores(ctx, "vlgp_loglik", us, vb, LoglikScorer{d_rate}, ctx->d_work, d_sums);
}
