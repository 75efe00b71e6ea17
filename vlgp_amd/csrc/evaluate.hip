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
// caller listed the channels, and evaluates that channel under that replica's posterior on the source rows.  The four
// sums of each (channel, workgroup) are reduced in a fixed order -- a butterfly over the wave, then the four waves in
// order -- into a partial per workgroup; ll_finish adds the partials of a channel in workgroup order.  No atomics: the
// sums are the same bits on every run.
#include "ctx.h"
#include "fast_exp.h"

namespace {

struct LlArgs {
    int N, L, n_blk;
    int64_t rows;          // rows per slot: the set's rows (plain) or the source's (replicated)
    const double* y;       // (rows, N)
    const double* xb;      // (rows, N) or null: then b[n] (x == 1)
    const double* b;
    const double* a;       // (L, N)
    const double* noise;
    const int* gauss;
    const double* mu;      // (rows_total, L)
    const double* v;
    int vb;
    const int* ch;         // replicated set: left-out channel of each pair, else null
    const int* pair_rep;   // replicated set: replica of each pair
    int n_pairs;
    double* rate;          // plain (rows, N), replicated (rows, n_pairs), or null
    double* part;          // (slots, n_blk, 4)
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ void __launch_bounds__(256) ll_rows(LlArgs A) {
    __shared__ double red[2][4][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < A.rows;
    const int64_t row = in ? r : 0;
    const int k = blockIdx.y;                       // pair (0 for a plain set)
    const int64_t mrow = (int64_t)(A.ch ? A.pair_rep[k] : 0) * A.rows + row;  // row of mu, v in the (replicated) set
    const int n0 = A.ch ? A.ch[k] : 0, n1 = A.ch ? n0 + 1 : A.N;
    for (int n = n0; n < n1; ++n) {
        double eta = A.xb ? A.xb[row * A.N + n] : A.b[n];
        for (int l = 0; l < A.L; ++l) eta = fma(A.mu[mrow * A.L + l], A.a[l * A.N + n], eta);
        const double yv = A.y[row * A.N + n];
        double s[4];
        if (A.gauss[n]) {
            const double nz = A.noise[n], d = yv - eta;
            s[0] = -0.5 * log(2.0 * M_PI * nz) - d * d / (2.0 * nz);
            s[2] = eta;
            s[3] = yv * yv;
            if (A.rate && in) A.rate[A.ch ? row * A.n_pairs + k : row * A.N + n] = eta;
        } else {
            if (A.vb)
                for (int l = 0; l < A.L; ++l) {
                    const double al = A.a[l * A.N + n];
                    eta = fma(A.v[mrow * A.L + l], 0.5 * al * al, eta);
                }
            const double lam = exp(clamp10(eta));
            const double lg = lgamma(yv + 1.0);
            s[0] = yv * log(lam) - lam - lg;
            s[2] = lam;
            s[3] = lg;
            if (A.rate && in) A.rate[A.ch ? row * A.n_pairs + k : row * A.N + n] = lam;
        }
        s[1] = yv;
        const int buf = n & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t = wave_sum(in ? s[j] : 0.0);
            if (lane == 0) red[buf][wid][j] = t;
        }
        __syncthreads();  // (two buffers: the next channel's writes cannot meet this channel's reads)
        if (threadIdx.x < 4) {
            const int j = threadIdx.x;
            const double t = ((red[buf][0][j] + red[buf][1][j]) + red[buf][2][j]) + red[buf][3][j];
            const int slot = A.ch ? k : n;
            A.part[((int64_t)slot * A.n_blk + blockIdx.x) * 4 + j] = t;
        }
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

int launch_loglik(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_rate, double* d_sums) {
    const bool rep = us.rep_src >= 0;
    const UnitSet& src = rep ? ctx->sets[us.rep_src] : us;
    LlArgs A;
    A.N = ctx->N; A.L = ctx->L;
    A.rows = rep ? us.rows_src : us.rows;
    A.n_blk = (int)((A.rows + 255) / 256);
    A.y = src.y;
    A.xb = src.x_ones ? nullptr : src.d_xb;
    A.b = ctx->d_b; A.a = ctx->d_a; A.noise = ctx->d_noise; A.gauss = ctx->d_gauss;
    A.mu = us.mu; A.v = us.v;
    A.vb = vb ? 1 : 0;
    A.ch = rep ? us.d_rep_ch : nullptr;
    A.pair_rep = rep ? us.d_rep_pair : nullptr;
    A.n_pairs = rep ? us.n_pairs : 0;
    A.rate = d_rate;
    const int slots = rep ? us.n_pairs : ctx->N;
    if (A.rows < 1 || A.n_blk < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_loglik on an empty set");
    if (rep && us.n_pairs > 65535)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_loglik: at most 65535 (replica, channel) pairs per set");
    CHK(vlgp_ensure_work(ctx, (int64_t)slots * A.n_blk * 4 + 8));
    A.part = ctx->d_work;
    hipLaunchKernelGGL(ll_rows, dim3((unsigned)A.n_blk, (unsigned)(rep ? us.n_pairs : 1)), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(ll_finish, dim3((unsigned)((slots * 4 + 255) / 256)), dim3(256), 0, ctx->stream, slots, A.n_blk,
                       ctx->d_work, d_sums);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
