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
// forecast_task: one wave per (unit, latent), everything in LDS, addressed through the prior table as elbo_kl (elbo.hip)
// addresses it.  Pass 1 over the rows of G in tiles of 64 accumulates G'WG (eight rows of the r x r result per lane in
// registers at a time, lane j owning column j) and G'z; a left-looking Cholesky (lane i owns row i) and the two triangular
// solves give beta; pass 2 over G, lane tt one row of the tile, the two convergence sums; pass 3 over G_ext, lane tt one
// row: its dot product with beta, then a forward substitution against Lc (read at wave-uniform addresses) in place in the
// lane's own tile row, and the squares of the columns >= r straight from global memory.  No atomics; every sum has a fixed
// order, so the outputs are the same bits on every run.  A pivot that is not positive and finite makes the task's
// outputs NaN and sets its flag; every index stays in bounds whatever the values are.
#include <algorithm>

#include "ctx.h"
#include "fast_exp.h"

namespace {

#define FC_LCH 8  // latents of g a lane holds in registers at a time

struct ForecastRowArgs {
    int N, L;
    int64_t rows;
    const double* y;       // (rows, N)
    const double* xb;      // (rows, N) or null: then b[n] (x == 1)
    const double* b;
    const double* a;       // (L, N)
    const double* noise;
    const int* gauss;
    const double* mu;      // (rows, L)
    const double* v;
    const double* w;
    int vb;
    double* z;             // (rows, L)
};

__global__ void __launch_bounds__(256) forecast_rows(ForecastRowArgs A) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= A.rows) return;
    for (int l0 = 0; l0 < A.L; l0 += FC_LCH) {
        double g[FC_LCH];
#pragma unroll
        for (int i = 0; i < FC_LCH; ++i) g[i] = 0.0;
        for (int n = 0; n < A.N; ++n) {
            double eta = A.xb ? A.xb[row * A.N + n] : A.b[n];
            for (int l = 0; l < A.L; ++l) eta = fma(A.mu[row * A.L + l], A.a[l * A.N + n], eta);
            const double yv = A.y[row * A.N + n];
            double res;
            if (A.gauss[n]) {
                res = (yv - eta) / A.noise[n];
            } else {
                double sv = 0.0;
                if (A.vb)
                    for (int l = 0; l < A.L; ++l) {
                        const double al = A.a[l * A.N + n];
                        sv = fma(A.v[row * A.L + l], 0.5 * al * al, sv);
                    }
                res = yv - exp(clamp10(eta + sv));
            }
#pragma unroll
            for (int i = 0; i < FC_LCH; ++i)
                if (l0 + i < A.L) g[i] = fma(A.a[(l0 + i) * A.N + n], res, g[i]);
        }
#pragma unroll
        for (int i = 0; i < FC_LCH; ++i)
            if (l0 + i < A.L) {
                const int64_t at = row * A.L + l0 + i;
                A.z[at] = fma(A.w[at], A.mu[at], g[i]);
            }
    }
}

// ---- task kernel ------------------------------------------------------------------------------------------------
#define FC_TILE 64   // rows of G (or G_ext) staged per step
#define FC_CH 8      // rows of the r x r accumulator a lane holds in registers at a time

struct ForecastTaskArgs {
    int L, M, R, rp, rs, vb;  // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp)
    const int64_t* off;       // (M + 1)
    const int* unit_prior;    // (M)
    const double* const* prior_base;
    const int* prior_rl;       // (table rows, L)
    const int64_t* prior_goff; // (table rows, L)
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
    // H | tile (+ FC_CH of slack: the register chunk may read past column r) | w | z | 1/diag Lc | beta
    return rp * rs + FC_TILE * rs + FC_CH + 2 * FC_TILE + 2 * rp;
}

__device__ __forceinline__ double fc_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ void fc_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// columns [0, r) of rows [t0, t0 + nt) of a row-major factor of row length ld into the tile, row stride rs
__device__ __forceinline__ void fc_stage(const double* __restrict__ G, int ld, int r, int rs, int t0, int nt, double* tile,
                                         int lane) {
    const double* src = G + (int64_t)t0 * ld;
    for (int e = lane; e < nt * r; e += 64) {
        const int tt = e / r, j = e - tt * r;
        tile[tt * rs + j] = src[(int64_t)tt * ld + j];
    }
}

__global__ void __launch_bounds__(64) forecast_task(ForecastTaskArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int task = blockIdx.x;
    const int u = task / A.L, l = task - u * A.L;
    if (u >= A.M) return;
    const int rp = A.rp, rs = A.rs;
    double* Hm = lds;
    double* tile = Hm + rp * rs;
    double* wv = tile + FC_TILE * rs + FC_CH;
    double* zv = wv + FC_TILE;
    double* dinv = zv + FC_TILE;
    double* bet = dinv + rp;

    const int64_t r0 = A.off[u];
    const int T = (int)(A.off[u + 1] - r0);
    const int64_t e0 = A.ext_off[u];
    const int nx = (int)(A.ext_off[u + 1] - e0);
    const int p = A.unit_prior[u];
    const int r = A.prior_rl[p * A.L + l];
    const double nan = __builtin_nan("");
    if (r < 1 || r > rp || r > A.R || T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        for (int t = lane; t < nx; t += 64) A.mu_ext[(e0 + t) * A.L + l] = A.v_ext[(e0 + t) * A.L + l] = nan;
        if (lane < 2) A.terms[(int64_t)task * 2 + lane] = nan;
        if (lane == 0) A.flag[task] = 1;
        return;
    }
    const double* __restrict__ G = A.prior_base[p] + A.prior_goff[p * A.L + l];
    const double* __restrict__ Gx = A.G_ext + A.gx_off[u] + (int64_t)l * nx * A.R;
    const int j = lane < r ? lane : 0;  // the lane's column (lanes >= r compute on column 0 and store nothing)

    for (int e = lane; e < rp * rs + FC_TILE * rs + FC_CH; e += 64) lds[e] = 0.0;
    fc_sync();

    // ---- pass 1: G'WG, G'z ----
    double cj = 0.0;
    for (int t0 = 0; t0 < T; t0 += FC_TILE) {
        const int nt = min(FC_TILE, T - t0);
        fc_stage(G, r, r, rs, t0, nt, tile, lane);
        if (lane < nt) {
            const int64_t at = (r0 + t0 + lane) * A.L + l;
            wv[lane] = A.w[at];
            zv[lane] = A.z[at];
        }
        fc_sync();
        for (int tt = 0; tt < nt; ++tt) cj = fma(tile[tt * rs + j], zv[tt], cj);
        for (int i0 = 0; i0 < r; i0 += FC_CH) {
            double aw[FC_CH];
#pragma unroll
            for (int i = 0; i < FC_CH; ++i) aw[i] = 0.0;
            for (int tt = 0; tt < nt; ++tt) {
                const double* trow = tile + tt * rs;
                const double wg = wv[tt] * trow[j];
#pragma unroll
                for (int i = 0; i < FC_CH; ++i)
                    aw[i] = fma(wg, trow[i0 + i], aw[i]);  // (wave-uniform address; past column r: the next row or the slack)
            }
            if (lane < r) {
#pragma unroll
                for (int i = 0; i < FC_CH; ++i)
                    if (i0 + i < r) Hm[(i0 + i) * rs + lane] += aw[i];
            }
        }
        fc_sync();  // (the tile is overwritten next)
    }
    if (lane < r) Hm[lane * rs + lane] += 1.0;
    fc_sync();

    // ---- H = Lc Lc': left-looking, lane i owning row i; the factor replaces the lower triangle ----
    int bad = 0;
    {
        const int row = lane < r ? lane : 0;
        for (int k = 0; k < r; ++k) {
            double s = Hm[row * rs + k];
            for (int q = 0; q < k; ++q) s = fma(-Hm[row * rs + q], Hm[k * rs + q], s);
            const double d = __shfl(s, k, 64);
            bad |= (!(d > 0.0) || !(d < 1e300)) ? 1 : 0;
            const double sd = sqrt(d);
            if (lane >= k && lane < r) Hm[lane * rs + k] = (lane == k) ? sd : s / sd;
            if (lane == k) dinv[k] = 1.0 / sd;
            fc_sync();
        }
    }

    // ---- beta = H^-1 G'z: forward and backward substitution, lane k holding entry k ----
    double bz = lane < r ? cj : 0.0;
    for (int k = 0; k < r; ++k) {
        const double zk = __shfl(bz, k, 64) * dinv[k];
        if (lane == k) bz = zk;
        else if (lane > k && lane < r) bz = fma(-Hm[lane * rs + k], zk, bz);
    }
    for (int k = r - 1; k >= 0; --k) {
        const double bk = __shfl(bz, k, 64) * dinv[k];
        if (lane == k) bz = bk;
        else if (lane < k) bz = fma(-Hm[k * rs + lane], bk, bz);
    }
    if (lane < r) bet[lane] = bz;
    fc_sync();

    // ---- pass 2: |G beta - mu|^2 and |mu|^2, lane tt one row of the tile ----
    double res = 0.0, msq = 0.0;
    for (int t0 = 0; t0 < T; t0 += FC_TILE) {
        const int nt = min(FC_TILE, T - t0);
        fc_stage(G, r, r, rs, t0, nt, tile, lane);
        fc_sync();
        if (lane < nt) {
            double gb = 0.0;
            for (int q = 0; q < r; ++q) gb = fma(tile[lane * rs + q], bet[q], gb);
            const double m = A.mu[(r0 + t0 + lane) * A.L + l];
            const double d = gb - m;
            res = fma(d, d, res);
            msq = fma(m, m, msq);
        }
        fc_sync();
    }
    const double resid = fc_wave_sum(res), musq = fc_wave_sum(msq);
    if (lane == 0) {
        A.terms[(int64_t)task * 2 + 0] = bad ? nan : resid;
        A.terms[(int64_t)task * 2 + 1] = bad ? nan : musq;
        A.flag[task] = bad ? 1 : 0;
    }

    // ---- pass 3: the extension rows, lane tt one row of the tile ----
    for (int t0 = 0; t0 < nx; t0 += FC_TILE) {
        const int nt = min(FC_TILE, nx - t0);
        fc_stage(Gx, A.R, r, rs, t0, nt, tile, lane);
        fc_sync();
        if (lane < nt) {
            double* xr = tile + lane * rs;
            double m = 0.0;
            for (int q = 0; q < r; ++q) m = fma(xr[q], bet[q], m);
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
            const int64_t at = (e0 + t0 + lane) * A.L + l;
            A.mu_ext[at] = bad ? nan : m;
            A.v_ext[at] = bad ? nan : var;
        }
        fc_sync();
    }
}

}  // namespace

// d_z: (rows, L) doubles of workspace; d_ext_off (M + 1), d_gx_off (M): see ForecastTaskArgs; d_mu_ext, d_v_ext
// (sum n_ext, L), d_terms (M, L, 2), d_flag (M, L)
int launch_forecast(vlgp_ctx* ctx, UnitSet& us, int vb, int rp, double* d_z, const int64_t* d_ext_off,
                    const int64_t* d_gx_off, const double* d_G_ext, double* d_mu_ext, double* d_v_ext, double* d_terms,
                    int* d_flag) {
    if (rp < 1 || rp > VLGP_WAVE || rp > ctx->R)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: effective rank %d outside [1, %d]", rp, std::min(VLGP_WAVE, ctx->R));
    ForecastTaskArgs K;
    K.L = ctx->L; K.M = us.M; K.R = ctx->R;
    K.rp = rp;
    K.rs = rp | 1;
    K.vb = vb ? 1 : 0;
    const size_t lds = sizeof(double) * (size_t)forecast_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_forecast: rank %d needs %zu bytes of LDS", rp, lds);

    ForecastRowArgs R;
    R.N = ctx->N; R.L = ctx->L;
    R.rows = us.rows;
    R.y = us.y;
    R.xb = us.x_ones ? nullptr : us.d_xb;
    R.b = ctx->d_b; R.a = ctx->d_a; R.noise = ctx->d_noise; R.gauss = ctx->d_gauss;
    R.mu = us.mu; R.v = us.v; R.w = us.w;
    R.vb = vb ? 1 : 0;
    R.z = d_z;
    hipLaunchKernelGGL(forecast_rows, dim3((unsigned)((us.rows + 255) / 256)), dim3(256), 0, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());

    K.off = us.d_off; K.unit_prior = us.d_unit_prior;
    K.prior_base = ctx->d_prior_base; K.prior_rl = ctx->d_prior_rl; K.prior_goff = ctx->d_prior_goff;
    K.mu = us.mu; K.w = us.w; K.z = d_z;
    K.ext_off = d_ext_off; K.gx_off = d_gx_off; K.G_ext = d_G_ext;
    K.mu_ext = d_mu_ext; K.v_ext = d_v_ext; K.terms = d_terms; K.flag = d_flag;
    if (lds > 64 * 1024 &&
        std::find(ctx->lds_attr_done.begin(), ctx->lds_attr_done.end(), (const void*)forecast_task) == ctx->lds_attr_done.end()) {
        HIPCHK(ctx, hipFuncSetAttribute((const void*)forecast_task, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_max));
        ctx->lds_attr_done.push_back((const void*)forecast_task);
    }
    hipLaunchKernelGGL(forecast_task, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
