// What the read-only evaluation calls share (evaluate.hip, elbo.hip, forecast.hip): the row model of their one-lane-per-row
// kernels, the fixed-order reduction of four sums per (channel, workgroup), and the steps of their one-wave-per-(unit,
// latent) kernels on a compact prior factor in LDS.  Device helpers and the host code that fills their arguments; no
// kernels.  Every sum has a fixed order and there are no atomics: the results are the same bits on every run.
#pragma once
#include "ctx.h"

#define EW_TILE 64  // rows of a factor staged per step
#define EW_CH 8     // rows of an r x r accumulator a lane holds in registers at a time

// ---- rows -----------------------------------------------------------------------------------------------------------
struct RowModel {
    int N, L, vb;
    int64_t rows;          // rows of y, xb: the set's own, or the source's for a replicated set
    const double* y;       // (rows, N)
    const double* xb;      // (rows, N) or null: then b[n] (x == 1)
    const double* b;
    const double* a;       // (L, N)
    const double* noise;
    const int* gauss;
    const double* mu;      // (rows of the posterior's set, L)
    const double* v;
};

// y, xb of `src`; mu, v of `post` (the same set, or the replicated set whose source `src` is)
static inline RowModel fill_row_model(const vlgp_ctx* ctx, const UnitSet& src, const UnitSet& post, int vb) {
    RowModel M;
    M.N = ctx->N; M.L = ctx->L; M.vb = vb ? 1 : 0;
    M.rows = src.rows;
    M.y = src.y;
    M.xb = src.x_ones ? nullptr : src.d_xb;
    M.b = ctx->d_b; M.a = ctx->d_a; M.noise = ctx->d_noise; M.gauss = ctx->d_gauss;
    M.mu = post.mu; M.v = post.v;
    return M;
}

// eta = (b x)_row,n + a_n . mu_mrow, one chain
__device__ __forceinline__ double row_eta(const RowModel& M, int64_t row, int64_t mrow, int n) {
    double eta = M.xb ? M.xb[row * M.N + n] : M.b[n];
    for (int l = 0; l < M.L; ++l) eta = fma(M.mu[mrow * M.L + l], M.a[l * M.N + n], eta);
    return eta;
}

// acc + 1/2 (a_n^2) . v_mrow, the chain started from acc (acc itself when vb == 0)
__device__ __forceinline__ double row_quad(const RowModel& M, int64_t mrow, int n, double acc) {
    if (M.vb)
        for (int l = 0; l < M.L; ++l) {
            const double al = M.a[l * M.N + n];
            acc = fma(M.v[mrow * M.L + l], 0.5 * al * al, acc);
        }
    return acc;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the four sums of channel n over a workgroup of 256 into part_slot[0 .. 3]: a butterfly over each wave, then the four
// waves in order.  Called by every thread; red alternates on n, so the next channel's writes cannot meet this one's reads.
__device__ __forceinline__ void block_sums4(const double (&s)[4], bool in, int n, double (*red)[4][4], double* part_slot) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, buf = n & 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double t = wave_sum(in ? s[j] : 0.0);
        if (lane == 0) red[buf][wid][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        part_slot[j] = ((red[buf][0][j] + red[buf][1][j]) + red[buf][2][j]) + red[buf][3][j];
    }
}

// ---- one wave per (unit, latent) ------------------------------------------------------------------------------------
struct TaskPrior {
    int L, M;
    const int64_t* off;        // (M + 1)
    const int* unit_prior;     // (M)
    const double* const* prior_base;
    const int* prior_rl;       // (table rows, L)
    const int64_t* prior_goff; // (table rows, L)
};

static inline TaskPrior fill_task_prior(const vlgp_ctx* ctx, const UnitSet& us) {
    return {ctx->L, us.M, us.d_off, us.d_unit_prior, ctx->d_prior_base, ctx->d_prior_rl, ctx->d_prior_goff};
}

struct TaskView {
    int u, l, T, p, r;     // unit, latent, the unit's length, its prior's table row, the latent's effective rank
    int64_t r0;            // the unit's first row
    const double* G;       // (T, r) compact factor
};

__device__ __forceinline__ TaskView task_view(const TaskPrior& P, int task) {
    TaskView t;
    t.u = task / P.L;
    t.l = task - t.u * P.L;
    t.r0 = P.off[t.u];
    t.T = (int)(P.off[t.u + 1] - t.r0);
    t.p = P.unit_prior[t.u];
    t.r = P.prior_rl[t.p * P.L + t.l];
    t.G = P.prior_base[t.p] + P.prior_goff[t.p * P.L + t.l];
    return t;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void wave_zero(double* lds, int n, int lane) {
    for (int e = lane; e < n; e += 64) lds[e] = 0.0;
    wave_sync();
}

// columns [0, r) of rows [t0, t0 + nt) of a row-major factor of row length ld into the tile, row stride rs
__device__ __forceinline__ void stage_rows(const double* __restrict__ G, int ld, int r, int rs, int t0, int nt, double* tile,
                                           int lane) {
    const double* src = G + (int64_t)t0 * ld;
    for (int e = lane; e < nt * r; e += 64) {
        const int tt = e / r, j = e - tt * r;
        tile[tt * rs + j] = src[(int64_t)tt * ld + j];
    }
}

// Hm += G' diag(wv) G (and Bm += G'G) over the nt staged rows: EW_CH rows of the r x r result per lane in registers at a
// time, lane j owning column j (lanes >= r compute on column 0 and store nothing)
template <bool WITH_GG>
__device__ __forceinline__ void accum_gwg(const double* tile, const double* wv, int nt, int r, int rs, int j, int lane,
                                          double* Hm, double* Bm) {
    for (int i0 = 0; i0 < r; i0 += EW_CH) {
        double aw[EW_CH], ag[EW_CH];
#pragma unroll
        for (int i = 0; i < EW_CH; ++i) aw[i] = ag[i] = 0.0;
        for (int tt = 0; tt < nt; ++tt) {
            const double* trow = tile + tt * rs;
            const double gj = trow[j], wg = wv[tt] * gj;
#pragma unroll
            for (int i = 0; i < EW_CH; ++i) {
                const double gi = trow[i0 + i];  // (wave-uniform address; past column r: the next row or the slack)
                aw[i] = fma(wg, gi, aw[i]);
                if (WITH_GG) ag[i] = fma(gj, gi, ag[i]);
            }
        }
        if (lane < r) {
#pragma unroll
            for (int i = 0; i < EW_CH; ++i)
                if (i0 + i < r) {
                    Hm[(i0 + i) * rs + lane] += aw[i];
                    if (WITH_GG) Bm[(i0 + i) * rs + lane] += ag[i];
                }
        }
    }
}

// left-looking Cholesky of the r x r matrix M (LDS, row stride rs), lane i owning row i; the factor replaces the lower
// triangle, dinv[k] = 1 / L[k][k].  Returns nonzero on a pivot that is not positive and finite.
__device__ __forceinline__ int wave_chol(double* M, int r, int rs, double* dinv, int lane) {
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
        wave_sync();
    }
    return bad;
}

// (Lc Lc')^-1 z by forward and backward substitution against the factor wave_chol left, lane k holding entry k
__device__ __forceinline__ double wave_solve_llt(const double* Lc, const double* dinv, int r, int rs, double z, int lane) {
    for (int k = 0; k < r; ++k) {
        const double zk = __shfl(z, k, 64) * dinv[k];
        if (lane == k) z = zk;
        else if (lane > k && lane < r) z = fma(-Lc[lane * rs + k], zk, z);
    }
    for (int k = r - 1; k >= 0; --k) {
        const double bk = __shfl(z, k, 64) * dinv[k];
        if (lane == k) z = bk;
        else if (lane < k) z = fma(-Lc[k * rs + lane], bk, z);
    }
    return z;
}

// The weight-space posterior of one (unit, latent), beta ~ N(m, H^-1): pass 1 over the rows of G in tiles of 64
// accumulates H = I_r + G' diag(w) G and G'z, then H = Lc Lc' (the factor in the lower triangle of Hm, dinv = 1 / diag Lc)
// and m = H^-1 G'z, lane k returning entry k.  lds (zeroed here): Hm | tile | wv | zv at the caller's offsets; w, z are
// the set's (rows, L) columns.  *bad: a pivot was not positive and finite.
__device__ __forceinline__ double task_weight_posterior(const TaskView& t, int L, const double* w, const double* z, int rs,
                                                        int lane, double* lds, int n_zero, double* Hm, double* tile,
                                                        double* wv, double* zv, double* dinv, int* bad) {
    const int T = t.T, r = t.r;
    const int j = lane < r ? lane : 0;  // the lane's column (lanes >= r compute on column 0 and store nothing)
    wave_zero(lds, n_zero, lane);
    double cj = 0.0;
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
        if (lane < nt) {
            const int64_t at = (t.r0 + t0 + lane) * L + t.l;
            wv[lane] = w[at];
            zv[lane] = z[at];
        }
        wave_sync();
        for (int tt = 0; tt < nt; ++tt) cj = fma(tile[tt * rs + j], zv[tt], cj);
        accum_gwg<false>(tile, wv, nt, r, rs, j, lane, Hm, nullptr);
        wave_sync();  // (the tile is overwritten next)
    }
    if (lane < r) Hm[lane * rs + lane] += 1.0;
    wave_sync();
    *bad = wave_chol(Hm, r, rs, dinv, lane);
    return wave_solve_llt(Hm, dinv, r, rs, lane < r ? cj : 0.0, lane);
}

// one staged row . beta
__device__ __forceinline__ double tile_row_dot(const double* trow, const double* bet, int r) {
    double g = 0.0;
    for (int q = 0; q < r; ++q) g = fma(trow[q], bet[q], g);
    return g;
}
