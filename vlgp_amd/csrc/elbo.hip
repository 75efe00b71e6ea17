// Variational lower bound of a unit set (vlgp_elbo): the expected log-likelihood per channel and the terms of
// KL[q(x_l) || p(x_l)] per (unit, latent).
//
// For one unit of length T and latent l, G (T x r) the compact prior factor, w, mu the unit's columns:
//   H = I_r + G' diag(w) G,  S = H^-1,  q(x_l) = N(mu, G S G'),  beta = argmin |G beta - mu|
//   KL = 1/2 (tr S + beta'beta - r + log det H)                      (assembled on the host, evaluation.elbo_from_terms)
// Expected log-likelihood of y[t, n], eta = a_n . mu_t + (b x)_tn, s = 1/2 (a_n^2) . v_t (0 when vb == 0):
//   Poisson   y eta - trunc_exp(eta + s) - lgamma(y + 1)             sums = E log p | y | rate | y s
//   Gaussian  -1/2 log(2 pi noise_n) - ((y - eta)^2 + 2 s) / (2 noise_n)   sums = E log p | y | eta | s / noise_n
//
// elbo_rows: one lane per row, the channels in plain order, the four sums of each (channel, workgroup) reduced as
// ll_rows (evaluate.hip) reduces its own -- a butterfly over the wave, the four waves in order, a partial per workgroup;
// elbo_finish adds the partials of a channel in workgroup order.  A lane also leaves the row's own sum over the
// channels (row_ell) when asked: the per-unit split of the expected log-likelihood is a host-side sum of those.
//
// elbo_kl: one wave per (unit, latent), everything in LDS.  One pass over the rows of G in tiles of 64 accumulates
// G'WG, G'G (eight rows of the r x r result per lane in registers at a time, lane j owning column j) and G'mu;
// then a left-looking Cholesky of both matrices (lane i owns row i), log det H from the diagonal, tr S = |L^-1|_F^2 with
// lane c solving for column c of L^-1 (kept in the unused upper triangle), the two triangular solves for beta, and a
// SECOND pass over G for |mu - G beta|^2 (the expanded form cancels to nothing near zero).  No atomics; every sum has a
// fixed order, so the terms are the same bits on every run.  A non-positive pivot makes the task's terms NaN and sets its
// flag; every index stays in bounds whatever the values are.
#include <algorithm>

#include "ctx.h"
#include "fast_exp.h"

namespace {

struct ElboRowArgs {
    int N, L, n_blk;
    int64_t rows;
    const double* y;       // (rows, N)
    const double* xb;      // (rows, N) or null: then b[n] (x == 1)
    const double* b;
    const double* a;       // (L, N)
    const double* noise;
    const int* gauss;
    const double* mu;      // (rows, L)
    const double* v;
    int vb;
    double* row_ell;       // (rows) or null
    double* part;          // (N, n_blk, 4)
};

__device__ __forceinline__ double elbo_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ void __launch_bounds__(256) elbo_rows(ElboRowArgs A) {
    __shared__ double red[2][4][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < A.rows;
    const int64_t row = in ? r : 0;
    double ell_row = 0.0;
    for (int n = 0; n < A.N; ++n) {
        double eta = A.xb ? A.xb[row * A.N + n] : A.b[n];
        for (int l = 0; l < A.L; ++l) eta = fma(A.mu[row * A.L + l], A.a[l * A.N + n], eta);
        double sv = 0.0;
        if (A.vb)
            for (int l = 0; l < A.L; ++l) {
                const double al = A.a[l * A.N + n];
                sv = fma(A.v[row * A.L + l], 0.5 * al * al, sv);
            }
        const double yv = A.y[row * A.N + n];
        double s[4];
        if (A.gauss[n]) {
            const double nz = A.noise[n], d = yv - eta;
            s[0] = -0.5 * log(2.0 * M_PI * nz) - (d * d + 2.0 * sv) / (2.0 * nz);
            s[2] = eta;
            s[3] = sv / nz;
        } else {
            const double lam = exp(clamp10(eta + sv));
            s[0] = yv * eta - lam - lgamma(yv + 1.0);
            s[2] = lam;
            s[3] = yv * sv;
        }
        s[1] = yv;
        ell_row += s[0];
        const int buf = n & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t = elbo_wave_sum(in ? s[j] : 0.0);
            if (lane == 0) red[buf][wid][j] = t;
        }
        __syncthreads();  // (two buffers: the next channel's writes cannot meet this channel's reads)
        if (threadIdx.x < 4) {
            const int j = threadIdx.x;
            const double t = ((red[buf][0][j] + red[buf][1][j]) + red[buf][2][j]) + red[buf][3][j];
            A.part[((int64_t)n * A.n_blk + blockIdx.x) * 4 + j] = t;
        }
    }
    if (A.row_ell && in) A.row_ell[r] = ell_row;
}

// sums[n][j] = the channel's partials added in workgroup order
__global__ void __launch_bounds__(256) elbo_finish(int slots, int n_blk, const double* __restrict__ part,
                                                   double* __restrict__ sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots * 4) return;
    const int slot = i >> 2, j = i & 3;
    double t = 0.0;
    for (int b = 0; b < n_blk; ++b) t += part[((int64_t)slot * n_blk + b) * 4 + j];
    sums[i] = t;
}

// ---- KL terms ---------------------------------------------------------------------------------------------------
#define ELBO_TILE 64   // rows of G staged per step
#define ELBO_CH 8      // rows of the r x r accumulators a lane holds in registers at a time

struct ElboKlArgs {
    int L, M, rp, rs;      // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp)
    const int64_t* off;    // (M + 1)
    const int* unit_prior; // (M)
    const double* const* prior_base;
    const int* prior_rl;       // (table rows, L)
    const int64_t* prior_goff; // (table rows, L)
    const double* mu;      // (rows, L)
    const double* w;
    double* out;           // (M, L, 4): log det H | tr S | beta'beta | |mu - G beta|^2
    int* flag;             // (M, L): 1 = a pivot was not positive
};

__host__ __device__ inline int elbo_kl_lds_doubles(int rp, int rs) {
    // H | G'G | tile (+ ELBO_CH of slack: the register chunk may read past column r) | w | mu | 1/diag H | 1/diag B | beta
    return 2 * rp * rs + ELBO_TILE * rs + ELBO_CH + 2 * ELBO_TILE + 3 * rp;
}

__device__ __forceinline__ void elbo_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// rows [t0, t0 + nt) of the compact factor into the tile, row stride rs (one contiguous, coalesced read)
__device__ __forceinline__ void elbo_stage(const double* __restrict__ G, int r, int rs, int t0, int nt, double* tile,
                                           int lane) {
    const double* src = G + (int64_t)t0 * r;
    for (int e = lane; e < nt * r; e += 64) {
        const int tt = e / r, j = e - tt * r;
        tile[tt * rs + j] = src[e];
    }
}

// left-looking Cholesky of the r x r matrix M (LDS, row stride rs), lane i owning row i; the factor replaces the lower
// triangle, dinv[k] = 1 / L[k][k].  Returns nonzero on a pivot that is not positive and finite.
__device__ __forceinline__ int elbo_chol(double* M, int r, int rs, double* dinv, int lane) {
    const int row = lane < r ? lane : 0;
    int bad = 0;
    for (int k = 0; k < r; ++k) {
        double s = M[row * rs + k];
        for (int q = 0; q < k; ++q) s = fma(-M[row * rs + q], M[k * rs + q], s);
        const double d = __shfl(s, k, 64);
        bad |= (!(d > 0.0) || !(d < 1e300)) ? 1 : 0;
        const double sd = sqrt(d);
        if (lane >= k && lane < r) M[lane * rs + k] = (lane == k) ? sd : s / sd;
        if (lane == k) dinv[k] = 1.0 / sd;
        elbo_sync();
    }
    return bad;
}

__global__ void __launch_bounds__(64) elbo_kl(ElboKlArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int task = blockIdx.x;
    const int u = task / A.L, l = task - u * A.L;
    if (u >= A.M) return;
    const int rp = A.rp, rs = A.rs;
    double* Hm = lds;
    double* Bm = Hm + rp * rs;
    double* tile = Bm + rp * rs;
    double* wv = tile + ELBO_TILE * rs + ELBO_CH;
    double* muv = wv + ELBO_TILE;
    double* dinvH = muv + ELBO_TILE;
    double* dinvB = dinvH + rp;
    double* bet = dinvB + rp;

    const int64_t r0 = A.off[u];
    const int T = (int)(A.off[u + 1] - r0);
    const int p = A.unit_prior[u];
    const int r = A.prior_rl[p * A.L + l];
    if (r < 1 || r > rp || T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        if (lane < 4) A.out[(int64_t)task * 4 + lane] = __builtin_nan("");
        if (lane == 0) A.flag[task] = 1;
        return;
    }
    const double* __restrict__ G = A.prior_base[p] + A.prior_goff[p * A.L + l];
    const int j = lane < r ? lane : 0;  // the lane's column (lanes >= r compute on column 0 and store nothing)

    for (int e = lane; e < 2 * rp * rs + ELBO_TILE * rs + ELBO_CH; e += 64) lds[e] = 0.0;
    elbo_sync();

    // ---- pass 1: G'WG, G'G, G'mu ----
    double cj = 0.0;
    for (int t0 = 0; t0 < T; t0 += ELBO_TILE) {
        const int nt = min(ELBO_TILE, T - t0);
        elbo_stage(G, r, rs, t0, nt, tile, lane);
        if (lane < nt) {
            const int64_t at = (r0 + t0 + lane) * A.L + l;
            wv[lane] = A.w[at];
            muv[lane] = A.mu[at];
        }
        elbo_sync();
        for (int tt = 0; tt < nt; ++tt) cj = fma(tile[tt * rs + j], muv[tt], cj);
        for (int i0 = 0; i0 < r; i0 += ELBO_CH) {
            double aw[ELBO_CH], ag[ELBO_CH];
#pragma unroll
            for (int i = 0; i < ELBO_CH; ++i) aw[i] = ag[i] = 0.0;
            for (int tt = 0; tt < nt; ++tt) {
                const double* trow = tile + tt * rs;
                const double gj = trow[j], wg = wv[tt] * gj;
#pragma unroll
                for (int i = 0; i < ELBO_CH; ++i) {
                    const double gi = trow[i0 + i];  // (wave-uniform address; past column r: the next row or the slack)
                    aw[i] = fma(wg, gi, aw[i]);
                    ag[i] = fma(gj, gi, ag[i]);
                }
            }
            if (lane < r) {
#pragma unroll
                for (int i = 0; i < ELBO_CH; ++i)
                    if (i0 + i < r) {
                        Hm[(i0 + i) * rs + lane] += aw[i];
                        Bm[(i0 + i) * rs + lane] += ag[i];
                    }
            }
        }
        elbo_sync();  // (the tile is overwritten next)
    }
    if (lane < r) Hm[lane * rs + lane] += 1.0;
    elbo_sync();

    // ---- factor both ----
    int bad = elbo_chol(Hm, r, rs, dinvH, lane);
    bad |= elbo_chol(Bm, r, rs, dinvB, lane);

    // log det H = 2 sum log L[k][k]
    const double logdet = 2.0 * elbo_wave_sum(lane < r ? log(Hm[lane * rs + lane]) : 0.0);

    // tr S = |L^-1|_F^2: lane c solves L x = e_c; x[i], i > c, kept at Hm[c][i] (the upper triangle, free after the factor)
    double tr = 0.0;
    {
        const int c = j;
        const double dc = dinvH[c];
        for (int i = 0; i < r; ++i) {
            double acc = 0.0;
            for (int q = 0; q < i; ++q) {
                const double lq = Hm[i * rs + q];
                const double xs = Hm[c * rs + q];  // (row c: its own lane's earlier writes, program order)
                const double xq = q > c ? xs : (q == c ? dc : 0.0);
                acc = fma(lq, xq, acc);
            }
            const double xi = ((i == c ? 1.0 : 0.0) - acc) * dinvH[i];
            if (lane < r && i > c) Hm[c * rs + i] = xi;
            asm volatile("" ::: "memory");
            tr = fma(xi, xi, tr);
        }
    }
    const double trS = elbo_wave_sum(lane < r ? tr : 0.0);

    // beta = (G'G)^-1 G'mu: forward and backward substitution, lane k holding entry k
    double z = lane < r ? cj : 0.0;
    for (int k = 0; k < r; ++k) {
        const double zk = __shfl(z, k, 64) * dinvB[k];
        if (lane == k) z = zk;
        else if (lane > k && lane < r) z = fma(-Bm[lane * rs + k], zk, z);
    }
    for (int k = r - 1; k >= 0; --k) {
        const double bk = __shfl(z, k, 64) * dinvB[k];
        if (lane == k) z = bk;
        else if (lane < k) z = fma(-Bm[k * rs + lane], bk, z);
    }
    const double bb = elbo_wave_sum(lane < r ? z * z : 0.0);
    if (lane < r) bet[lane] = z;
    elbo_sync();

    // ---- pass 2: |mu - G beta|^2, lane tt one row of the tile ----
    double res = 0.0;
    for (int t0 = 0; t0 < T; t0 += ELBO_TILE) {
        const int nt = min(ELBO_TILE, T - t0);
        elbo_stage(G, r, rs, t0, nt, tile, lane);
        elbo_sync();
        if (lane < nt) {
            double g = 0.0;
            for (int q = 0; q < r; ++q) g = fma(tile[lane * rs + q], bet[q], g);
            const double d = A.mu[(r0 + t0 + lane) * A.L + l] - g;
            res = fma(d, d, res);
        }
        elbo_sync();
    }
    const double resid = elbo_wave_sum(res);
    if (lane == 0) {
        const double nan = __builtin_nan("");
        double* o = A.out + (int64_t)task * 4;
        o[0] = bad ? nan : logdet;
        o[1] = bad ? nan : trS;
        o[2] = bad ? nan : bb;
        o[3] = bad ? nan : resid;
        A.flag[task] = bad ? 1 : 0;
    }
}

}  // namespace

// d_sums (N, 4), d_row_ell (rows) or null, d_terms (M, L, 4), d_flag (M, L); d_part: (N, n_blk, 4) doubles of workspace
int launch_elbo(vlgp_ctx* ctx, UnitSet& us, int vb, int rp, double* d_part, double* d_sums, double* d_row_ell,
                double* d_terms, int* d_flag) {
    ElboRowArgs R;
    R.N = ctx->N; R.L = ctx->L;
    R.rows = us.rows;
    R.n_blk = (int)((us.rows + 255) / 256);
    R.y = us.y;
    R.xb = us.x_ones ? nullptr : us.d_xb;
    R.b = ctx->d_b; R.a = ctx->d_a; R.noise = ctx->d_noise; R.gauss = ctx->d_gauss;
    R.mu = us.mu; R.v = us.v;
    R.vb = vb ? 1 : 0;
    R.row_ell = d_row_ell;
    R.part = d_part;
    hipLaunchKernelGGL(elbo_rows, dim3((unsigned)R.n_blk), dim3(256), 0, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(elbo_finish, dim3((unsigned)((ctx->N * 4 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->N, R.n_blk,
                       d_part, d_sums);
    HIPCHK(ctx, hipGetLastError());

    ElboKlArgs K;
    K.L = ctx->L; K.M = us.M;
    K.rp = rp;
    K.rs = rp | 1;
    K.off = us.d_off; K.unit_prior = us.d_unit_prior;
    K.prior_base = ctx->d_prior_base; K.prior_rl = ctx->d_prior_rl; K.prior_goff = ctx->d_prior_goff;
    K.mu = us.mu; K.w = us.w;
    K.out = d_terms; K.flag = d_flag;
    if (rp < 1 || rp > VLGP_WAVE) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_elbo: effective rank %d outside [1, %d]", rp, VLGP_WAVE);
    const size_t lds = sizeof(double) * (size_t)elbo_kl_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_elbo: rank %d needs %zu bytes of LDS", rp, lds);
    if (lds > 64 * 1024 &&
        std::find(ctx->lds_attr_done.begin(), ctx->lds_attr_done.end(), (const void*)elbo_kl) == ctx->lds_attr_done.end()) {
        HIPCHK(ctx, hipFuncSetAttribute((const void*)elbo_kl, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_max));
        ctx->lds_attr_done.push_back((const void*)elbo_kl);
    }
    hipLaunchKernelGGL(elbo_kl, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
