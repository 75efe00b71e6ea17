// Forward prediction of a unit set (vlgp_forecast): the posterior of every (unit, latent) carried past the unit's last row
// along further rows of the same prior factorisation.
//
// For one unit of length T and latent l, G (T x r) the compact prior factor, mu, v, w the unit's columns, G_ext (n_ext x R)
// the rows of the same factorisation at the unobserved bins:
//   g[t] = sum_n a[l, n] res[t, n],   res = y - exp(min(eta + 1/2 (a^2).v, 10)) (Poisson) | (y - eta) / noise (Gaussian)
//   z = g + w o mu,   H = I_r + G' diag(w) G = Lc Lc',   beta = H^-1 G' z          (G beta: the next unclipped Newton iterate)
//   mu_ext = G_ext[:, :r] beta,   v_ext[t] = |Lc^-1 G_ext[t, :r]'|^2 + sum_{c >= r} G_ext[t, c]^2   (0 when vb == 0)
//   fit_terms = {|G beta - mu|^2, |mu|^2}
//
// forecast_rows: one lane per row, the channels in plain order, eight latents of g in registers at a time (a set with more
// latents walks its channels once per eight); z goes to a (rows, L) workspace.
//
// forecast_task: one wave per (unit, latent), everything in LDS, built from the steps of eval_wave.h.  Pass 1 over the
// rows of G in tiles of 64 accumulates G'WG and G'z; the Cholesky and the two triangular solves give beta; pass 2 over G,
// lane tt one row of the tile, the two convergence sums; pass 3 over G_ext, lane tt one row: its dot product with beta,
// then a forward substitution against Lc (read at wave-uniform addresses) in place in the lane's own tile row, and the
// squares of the columns >= r straight from global memory.  A pivot that is not positive and finite makes the task's
// outputs NaN and sets its flag; every index stays in bounds whatever the values are.
#include <algorithm>

#include "eval_wave.h"
#include "fast_exp.h"

namespace {

#define FC_LCH 8  // latents of g a lane holds in registers at a time

struct ForecastRowArgs {
    RowModel m;
    const double* w;
    double* z;             // (rows, L)
};

__global__ void __launch_bounds__(256) forecast_rows(ForecastRowArgs A) {
    const RowModel& M = A.m;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= M.rows) return;
    for (int l0 = 0; l0 < M.L; l0 += FC_LCH) {
        double g[FC_LCH];
#pragma unroll
        for (int i = 0; i < FC_LCH; ++i) g[i] = 0.0;
        for (int n = 0; n < M.N; ++n) {
            const double eta = row_eta(M, row, row, n);
            const double yv = M.y[row * M.N + n];
            double res;
            if (M.gauss[n]) {
                res = (yv - eta) / M.noise[n];
            } else {
                const double sv = row_quad(M, row, n, 0.0);
                res = yv - exp(clamp10(eta + sv));
            }
#pragma unroll
            for (int i = 0; i < FC_LCH; ++i)
                if (l0 + i < M.L) g[i] = fma(M.a[(l0 + i) * M.N + n], res, g[i]);
        }
#pragma unroll
        for (int i = 0; i < FC_LCH; ++i)
            if (l0 + i < M.L) {
                const int64_t at = row * M.L + l0 + i;
                A.z[at] = fma(A.w[at], M.mu[at], g[i]);
            }
    }
}

// ---- task kernel ------------------------------------------------------------------------------------------------
struct ForecastTaskArgs {
    TaskPrior P;
    int R, rp, rs, vb;        // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp)
    const double* mu;         // (rows, L)
    const double* w;
    const double* z;
    const int64_t* ext_off;   // (M + 1): first extension row of each unit in mu_ext, v_ext
    const int64_t* gx_off;    // (M): offset (doubles) of the (L, n_ext, R) block of the unit's length inside G_ext
    const double* G_ext;
    double* mu_ext;           // (sum n_ext, L)
    double* v_ext;
    double* terms;            // (M, L, 2): |G beta - mu|^2 | |mu|^2
    int* flag;                // (M, L): 1 = a pivot was not positive and finite
};

__host__ __device__ inline int forecast_lds_doubles(int rp, int rs) {
    // H | tile (+ EW_CH of slack: the register chunk may read past column r) | w | z | 1/diag Lc | beta
    return rp * rs + EW_TILE * rs + EW_CH + 2 * EW_TILE + 2 * rp;
}

__global__ void __launch_bounds__(64) forecast_task(ForecastTaskArgs A) {
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
    double* bet = dinv + rp;

    const TaskView t = task_view(A.P, task);
    const int T = t.T, r = t.r, l = t.l;
    const int64_t r0 = t.r0, e0 = A.ext_off[t.u];
    const int nx = (int)(A.ext_off[t.u + 1] - e0);
    const double nan = __builtin_nan("");
    if (r < 1 || r > rp || r > A.R || T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        for (int i = lane; i < nx; i += 64) A.mu_ext[(e0 + i) * L + l] = A.v_ext[(e0 + i) * L + l] = nan;
        if (lane < 2) A.terms[(int64_t)task * 2 + lane] = nan;
        if (lane == 0) A.flag[task] = 1;
        return;
    }
    const double* __restrict__ Gx = A.G_ext + A.gx_off[t.u] + (int64_t)l * nx * A.R;

    // ---- pass 1: G'WG, G'z; H = Lc Lc', beta = H^-1 G'z ----
    int bad;
    const double bz = task_weight_posterior(t, L, A.w, A.z, rs, lane, lds, rp * rs + EW_TILE * rs + EW_CH, Hm, tile, wv, zv,
                                            dinv, &bad);
    if (lane < r) bet[lane] = bz;
    wave_sync();

    // ---- pass 2: |G beta - mu|^2 and |mu|^2, lane tt one row of the tile ----
    double res = 0.0, msq = 0.0;
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
        wave_sync();
        if (lane < nt) {
            const double gb = tile_row_dot(tile + lane * rs, bet, r);
            const double m = A.mu[(r0 + t0 + lane) * L + l];
            const double d = gb - m;
            res = fma(d, d, res);
            msq = fma(m, m, msq);
        }
        wave_sync();
    }
    const double resid = wave_sum(res), musq = wave_sum(msq);
    if (lane == 0) {
        A.terms[(int64_t)task * 2 + 0] = bad ? nan : resid;
        A.terms[(int64_t)task * 2 + 1] = bad ? nan : musq;
        A.flag[task] = bad ? 1 : 0;
    }

    // ---- pass 3: the extension rows, lane tt one row of the tile ----
    for (int t0 = 0; t0 < nx; t0 += EW_TILE) {
        const int nt = min(EW_TILE, nx - t0);
        stage_rows(Gx, A.R, r, rs, t0, nt, tile, lane);
        wave_sync();
        if (lane < nt) {
            double* xr = tile + lane * rs;
            const double m = tile_row_dot(xr, bet, r);
            double var = 0.0;
            if (A.vb) {
                for (int i = 0; i < r; ++i) {  // x = Lc^-1 (the row), in place: entry i is read before it is replaced
                    double s = xr[i];
                    for (int q = 0; q < i; ++q) s = fma(-Hm[i * rs + q], xr[q], s);
                    s *= dinv[i];
                    xr[i] = s;
                    var = fma(s, s, var);
                }
                const double* grow = Gx + (int64_t)(t0 + lane) * A.R;
                for (int c = r; c < A.R; ++c) var = fma(grow[c], grow[c], var);  // weights the data never saw: prior variance 1
            }
            const int64_t at = (e0 + t0 + lane) * L + l;
            A.mu_ext[at] = bad ? nan : m;
            A.v_ext[at] = bad ? nan : var;
        }
        wave_sync();
    }
}

}  // namespace

// z = g + w o mu of every (row, latent) into d_z (rows, L): the row pass, which vlgp_marginal shares
int launch_forecast_z(vlgp_ctx* ctx, UnitSet& us, int vb, double* d_z) {
    ForecastRowArgs R;
    R.m = fill_row_model(ctx, us, us, vb);
    R.w = us.w;
    R.z = d_z;
    hipLaunchKernelGGL(forecast_rows, dim3((unsigned)((us.rows + 255) / 256)), dim3(256), 0, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// d_z: (rows, L) doubles of workspace; d_ext_off (M + 1), d_gx_off (M): see ForecastTaskArgs; d_mu_ext, d_v_ext
// (sum n_ext, L), d_terms (M, L, 2), d_flag (M, L)
int launch_forecast(vlgp_ctx* ctx, UnitSet& us, int vb, int rp, double* d_z, const int64_t* d_ext_off,
                    const int64_t* d_gx_off, const double* d_G_ext, double* d_mu_ext, double* d_v_ext, double* d_terms,
                    int* d_flag) {
    if (rp < 1 || rp > VLGP_WAVE || rp > ctx->R)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: effective rank %d outside [1, %d]", rp, std::min(VLGP_WAVE, ctx->R));
    ForecastTaskArgs K;
    K.P = fill_task_prior(ctx, us);
    K.R = ctx->R;
    K.rp = rp;
    K.rs = rp | 1;
    K.vb = vb ? 1 : 0;
    const size_t lds = sizeof(double) * (size_t)forecast_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: rank %d needs %zu bytes of LDS", rp, lds);

    CHK(launch_forecast_z(ctx, us, vb, d_z));

    K.mu = us.mu; K.w = us.w; K.z = d_z;
    K.ext_off = d_ext_off; K.gx_off = d_gx_off; K.G_ext = d_G_ext;
    K.mu_ext = d_mu_ext; K.v_ext = d_v_ext; K.terms = d_terms; K.flag = d_flag;
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)forecast_task, ctx->lds_max));
    hipLaunchKernelGGL(forecast_task, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
