// Importance weights of a unit set (vlgp_marginal): the model's joint log density under K draws of every latent path of
// every unit from the fitted posterior, against the density of the draw -- the summands of the IWAE estimate of
// log p(y_unit).
//
// For one unit of length T and latent l, G (T x r) the compact prior factor, mu, v, w the unit's columns and z = g + w o mu
// (forecast.hip's row pass):
//   H = I_r + G' diag(w) G = Lc Lc',   m = H^-1 G' z                              (vlgp_forecast's weight-space posterior)
//   draw k:  d = Lc^-T eps_k,  beta_k = m + d,  x_k[t, l] = G[t, :] . beta_k
//   c[u, l, k] = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H                   (log N(beta; 0, I) - log N(beta; m, H^-1))
//   ll[u, k] = sum_t sum_n log p(y[t, n] | eta = a[:, n] . x_k[t] + (b x)_tn)     (no v term: x_k is a sample)
//   log_w[u, k] = ll[u, k] + sum_l c[u, l, k]
//
// marginal_task: one wave per (unit, latent), everything in LDS, built from the steps of eval_wave.h.  The first pass, the
// Cholesky and the solves of forecast_task give m, Lc and log det H; then one lane per sample: eps_k into the lane's own
// tile row, the back substitution against Lc' in place (Lc read at wave-uniform addresses), beta_k to the workspace with
// the sample index contiguous, and c.  A pivot that is not positive and finite makes c NaN (and with it the unit's log_w)
// and sets the task's flag; every index stays in bounds whatever the values are.
//
// marginal_rows: one wave per (unit, tile of rows), one lane per sample.  The paths of the tile first, x_k[t, l] for every
// latent into LDS (G at wave-uniform addresses, one coalesced load of beta per MR_ROWS FMAs); then the rows in order and
// the channels in order, y, (b x) and a wave-uniform, each lane adding its own sample's terms: no cross-lane reduction.
// What a term holds that no sample changes (lgamma(y + 1), the Gaussian constant) is added once per tile: the lanes share
// its entries and a butterfly adds them.  One software fp64 exp per (row, channel, sample) against L FMAs.
//
// marginal_finish: per (unit, sample) the tile partials in tile order, then the c of the latents in order.  No atomics:
// the same bits on every run, and a sample's numbers do not depend on its lane or on the samples beside it.
#include <algorithm>

#include "eval_wave.h"
#include "fast_exp.h"

#define MR_ROWS 8          // most rows a tile holds: the paths of a tile are MR_ROWS accumulators per latent
#define MR_LDS_ROWS 32     // a tile's paths take at most MR_LDS_ROWS * 64 doubles of LDS (16 KB)

int marginal_tile_rows(int L) { return std::max(1, std::min(MR_ROWS, MR_LDS_ROWS / std::max(L, 1))); }

namespace {

struct MarginalTaskArgs {
    TaskPrior P;
    int R, rp, rs, kc;        // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp); kc: samples
    const double* w;          // (rows, L)
    const double* z;
    const double* eps;        // (M, L, R, 64)
    double* beta;             // (M, L, R, 64)
    double* c;                // (M, L, 64)
    int* flag;                // (M, L): 1 = a pivot was not positive and finite
};

__host__ __device__ inline int marginal_lds_doubles(int rp, int rs) {
    // H | tile (+ EW_CH of slack: the register chunk may read past column r) | w | z | 1/diag Lc | m
    return rp * rs + EW_TILE * rs + EW_CH + 2 * EW_TILE + 2 * rp;
}

__global__ void __launch_bounds__(64) marginal_task(MarginalTaskArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int task = blockIdx.x;
    if (task >= A.P.M * A.P.L) return;
    const int rp = A.rp, rs = A.rs, L = A.P.L;
    double* Hm = lds;
    double* tile = Hm + rp * rs;
    double* wv = tile + EW_TILE * rs + EW_CH;
    double* zv = wv + EW_TILE;
    double* dinv = zv + EW_TILE;
    double* mean = dinv + rp;

    const TaskView t = task_view(A.P, task);
    const int r = t.r;
    const bool live = lane < A.kc;
    const double nan = __builtin_nan("");
    if (r < 1 || r > rp || r > A.R || t.T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        if (live) A.c[(int64_t)task * 64 + lane] = nan;
        if (lane == 0) A.flag[task] = 1;
        return;
    }
    int bad;
    const double mz = task_weight_posterior(t, L, A.w, A.z, rs, lane, lds, rp * rs + EW_TILE * rs + EW_CH, Hm, tile, wv, zv,
                                            dinv, &bad);
    if (lane < r) mean[lane] = mz;
    const double half_logdet = wave_sum(lane < r ? log(Hm[lane * rs + lane]) : 0.0);
    wave_sync();
    if (lane == 0) A.flag[task] = bad ? 1 : 0;

    // ---- the draws, lane k one sample (a lane past kc works on sample 0 and stores nothing) ----
    const int k = live ? lane : 0;
    const double* __restrict__ ek = A.eps + (int64_t)task * A.R * 64 + k;
    double* bk = A.beta + (int64_t)task * A.R * 64 + k;
    double* xr = tile + lane * rs;
    double e2 = 0.0;
    for (int i = 0; i < r; ++i) {
        const double e = ek[(int64_t)i * 64];
        xr[i] = e;
        e2 = fma(e, e, e2);
    }
    for (int i = r - 1; i >= 0; --i) {  // d = Lc^-T eps, in place: entry i is read before it is replaced
        double s = xr[i];
        for (int q = i + 1; q < r; ++q) s = fma(-Hm[q * rs + i], xr[q], s);
        xr[i] = s * dinv[i];
    }
    double b2 = 0.0;
    for (int i = 0; i < r; ++i) {
        const double bt = mean[i] + xr[i];
        b2 = fma(bt, bt, b2);
        if (live) bk[(int64_t)i * 64] = bt;
    }
    if (live) A.c[(int64_t)task * 64 + lane] = bad ? nan : (0.5 * e2 - 0.5 * b2) - half_logdet;
}

// ---- the hot kernel ---------------------------------------------------------------------------------------------
struct MarginalRowArgs {
    RowModel m;               // (mu, v are not read)
    TaskPrior P;
    int R, tile_rows;
    const int64_t* tile_off;  // (M + 1): first tile of each unit
    const double* beta;       // (M, L, R, 64)
    double* part;             // (tiles, 64)
};

__global__ void __launch_bounds__(64) marginal_rows(MarginalRowArgs A) {
    extern __shared__ double xs[];  // (tile_rows, L, 64): the paths of the tile, lane k its own column
    const RowModel& M = A.m;
    const int lane = threadIdx.x, L = M.L, N = M.N;
    const int64_t blk = blockIdx.x;
    int u = 0;
    for (int hi = A.P.M; hi - u > 1;) {  // the unit whose tiles hold blk: tile_off[u] <= blk < tile_off[u + 1]
        const int mid = u + (hi - u) / 2;
        if (A.tile_off[mid] <= blk) u = mid; else hi = mid;
    }
    const int64_t r0 = A.P.off[u];
    const int T = (int)(A.P.off[u + 1] - r0);
    const int t0 = (int)(blk - A.tile_off[u]) * A.tile_rows;
    const int nt = min(min(A.tile_rows, MR_ROWS), T - t0);
    if (nt < 1) return;  // (the host counted the tiles from the same lengths: never taken)
    const int p = A.P.unit_prior[u];

    // ---- the paths: x[tt, l] = G_l[t0 + tt, :] . beta_l ----
    for (int l = 0; l < L; ++l) {
        int r = A.P.prior_rl[p * L + l];
        if (r < 1 || r > A.R) r = 0;  // (marginal_task flagged it)
        const double* __restrict__ G = A.P.prior_base[p] + A.P.prior_goff[p * L + l] + (int64_t)t0 * r;
        const double* __restrict__ bk = A.beta + ((int64_t)u * L + l) * A.R * 64 + lane;
        double x[MR_ROWS];
#pragma unroll
        for (int i = 0; i < MR_ROWS; ++i) x[i] = 0.0;
        for (int q = 0; q < r; ++q) {
            const double bq = bk[(int64_t)q * 64];
#pragma unroll
            for (int i = 0; i < MR_ROWS; ++i)
                if (i < nt) x[i] = fma(G[i * r + q], bq, x[i]);
        }
#pragma unroll
        for (int i = 0; i < MR_ROWS; ++i)
            if (i < nt) xs[(i * L + l) * 64 + lane] = x[i];
    }

    // ---- what no sample changes: -lgamma(y + 1) | -1/2 log(2 pi noise), the tile's entries shared among the lanes ----
    double cst = 0.0;
    for (int e = lane; e < nt * N; e += 64) {
        const int tt = e / N, n = e - tt * N;
        cst -= M.gauss[n] ? 0.5 * log(2.0 * M_PI * M.noise[n]) : lgamma(M.y[(r0 + t0 + tt) * N + n] + 1.0);
    }
    cst = wave_sum(cst);

    // ---- the rows in order, the channels in order ----
    double acc = 0.0;
    for (int tt = 0; tt < nt; ++tt) {
        const int64_t row = r0 + t0 + tt;
        const double* xl = xs + tt * L * 64 + lane;
        for (int n = 0; n < N; ++n) {
            double eta = M.xb ? M.xb[row * N + n] : M.b[n];
            for (int l = 0; l < L; ++l) eta = fma(xl[l * 64], M.a[l * N + n], eta);
            const double yv = M.y[row * N + n];
            if (M.gauss[n]) {
                const double d = yv - eta;
                acc -= d * d / (2.0 * M.noise[n]);
            } else {
                acc += yv * eta - exp(clamp10(eta));
            }
        }
    }
    A.part[blk * 64 + lane] = acc + cst;
}

struct MarginalFinishArgs {
    int M, L, kc;
    const int64_t* tile_off;
    const double* part;
    const double* c;
    double* logw;             // (M, 64)
    double* parts;            // (M, 64, 2)
};

__global__ void __launch_bounds__(64) marginal_finish(MarginalFinishArgs A) {
    const int u = blockIdx.x, k = threadIdx.x;
    if (u >= A.M || k >= A.kc) return;
    double ll = 0.0, cs = 0.0;
    for (int64_t b = A.tile_off[u]; b < A.tile_off[u + 1]; ++b) ll += A.part[b * 64 + k];
    for (int l = 0; l < A.L; ++l) cs += A.c[((int64_t)u * A.L + l) * 64 + k];
    A.logw[(int64_t)u * 64 + k] = ll + cs;
    A.parts[((int64_t)u * 64 + k) * 2 + 0] = ll;
    A.parts[((int64_t)u * 64 + k) * 2 + 1] = cs;
}

}  // namespace

// the row kernel and the finish alone, for draws d_beta (M, L, R, 64) with their c in d_c (M, L, 64) already in place:
// launch_marginal's second half, which vlgp_joint_laplace shares (its draws come from joint.hip)
int launch_marginal_rows(vlgp_ctx* ctx, UnitSet& us, const char* who, int kc, const double* d_beta, const double* d_c,
                         double* d_part, int tile_rows, const int64_t* d_tile_off, int64_t n_tiles, double* d_logw,
                         double* d_parts) {
    if (kc < 1 || kc > 64 || tile_rows < 1 || tile_rows > MR_ROWS || n_tiles < 1 || n_tiles > 0x7fffffffLL)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: %d samples in %lld tiles of %d rows", who, kc, (long long)n_tiles, tile_rows);
    MarginalRowArgs R;
    R.m = fill_row_model(ctx, us, us, 0);
    R.P = fill_task_prior(ctx, us);
    R.R = ctx->R; R.tile_rows = tile_rows;
    R.tile_off = d_tile_off; R.beta = d_beta; R.part = d_part;
    const size_t xs = sizeof(double) * 64 * (size_t)tile_rows * ctx->L;
    if ((int64_t)xs > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: %d latents need %zu bytes of LDS", who, ctx->L, xs);
    if (xs > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)marginal_rows, ctx->lds_max));
    hipLaunchKernelGGL(marginal_rows, dim3((unsigned)n_tiles), dim3(64), xs, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());

    MarginalFinishArgs F = {us.M, ctx->L, kc, d_tile_off, d_part, d_c, d_logw, d_parts};
    hipLaunchKernelGGL(marginal_finish, dim3((unsigned)us.M), dim3(64), 0, ctx->stream, F);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

int launch_marginal(vlgp_ctx* ctx, UnitSet& us, int rp, int kc, const double* d_z, const double* d_eps, double* d_beta,
                    double* d_c, double* d_part, int tile_rows, const int64_t* d_tile_off, int64_t n_tiles, double* d_logw,
                    double* d_parts, int* d_flag) {
    if (rp < 1 || rp > VLGP_WAVE || rp > ctx->R)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_marginal: effective rank %d outside [1, %d]", rp, std::min(VLGP_WAVE, ctx->R));
    if (kc < 1 || kc > 64 || tile_rows < 1 || tile_rows > MR_ROWS || n_tiles < 1 || n_tiles > 0x7fffffffLL)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_marginal: %d samples in %lld tiles of %d rows", kc, (long long)n_tiles, tile_rows);
    MarginalTaskArgs K;
    K.P = fill_task_prior(ctx, us);
    K.R = ctx->R; K.rp = rp; K.rs = rp | 1; K.kc = kc;
    K.w = us.w; K.z = d_z; K.eps = d_eps; K.beta = d_beta; K.c = d_c; K.flag = d_flag;
    const size_t lds = sizeof(double) * (size_t)marginal_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_marginal: rank %d needs %zu bytes of LDS", rp, lds);
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)marginal_task, ctx->lds_max));
    hipLaunchKernelGGL(marginal_task, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return launch_marginal_rows(ctx, us, "vlgp_marginal", kc, d_beta, d_c, d_part, tile_rows, d_tile_off, n_tiles, d_logw, d_parts);
}
