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
// elbo_rows: one lane per row, the channels in plain order, a partial of the four sums per (channel, workgroup)
// (block_sums4) and then evaluate.hip's finish kernel.  A lane also leaves the row's own sum over the channels (row_ell)
// when asked: the per-unit split of the expected log-likelihood is a host-side sum of those.
//
// elbo_kl: one wave per (unit, latent), everything in LDS, built from the steps of eval_wave.h.  One pass over the rows of
// G in tiles of 64 accumulates G'WG, G'G and G'mu; then the Cholesky of both matrices, log det H from the diagonal,
// tr S = |L^-1|_F^2 with lane c solving for column c of L^-1 (kept in the unused upper triangle), the two triangular
// solves for beta, and a SECOND pass over G for |mu - G beta|^2 (the expanded form cancels to nothing near zero).  A
// non-positive pivot makes the task's terms NaN and sets its flag; every index stays in bounds whatever the values are.
#include "eval_wave.h"
#include "fast_exp.h"

namespace {

struct ElboRowArgs {
    RowModel m;
    int n_blk;
    double* row_ell;       // (rows) or null
    double* part;          // (N, n_blk, 4)
};

__global__ void __launch_bounds__(256) elbo_rows(ElboRowArgs A) {
    __shared__ double red[2][4][4];
    const RowModel& M = A.m;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < M.rows;
    const int64_t row = in ? r : 0;
    double ell_row = 0.0;
    for (int n = 0; n < M.N; ++n) {
        const double eta = row_eta(M, row, row, n);
        const double sv = row_quad(M, row, n, 0.0);
        const double yv = M.y[row * M.N + n];
        double s[4];
        if (M.gauss[n]) {
            const double nz = M.noise[n], d = yv - eta;
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
        block_sums4(s, in, n, red, A.part + ((int64_t)n * A.n_blk + blockIdx.x) * 4);
    }
    if (A.row_ell && in) A.row_ell[r] = ell_row;
}

// ---- KL terms ---------------------------------------------------------------------------------------------------
struct ElboKlArgs {
    TaskPrior P;
    int rp, rs;            // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp)
    const double* mu;      // (rows, L)
    const double* w;
    double* out;           // (M, L, 4): log det H | tr S | beta'beta | |mu - G beta|^2
    int* flag;             // (M, L): 1 = a pivot was not positive
};

__host__ __device__ inline int elbo_kl_lds_doubles(int rp, int rs) {
    // H | G'G | tile (+ EW_CH of slack: the register chunk may read past column r) | w | mu | 1/diag H | 1/diag B | beta
    return 2 * rp * rs + EW_TILE * rs + EW_CH + 2 * EW_TILE + 3 * rp;
}

__global__ void __launch_bounds__(64) elbo_kl(ElboKlArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int task = blockIdx.x;
    if (task >= A.P.M * A.P.L) return;
    const int rp = A.rp, rs = A.rs, L = A.P.L;
    double* Hm = lds;
    double* Bm = Hm + rp * rs;
    double* tile = Bm + rp * rs;
    double* wv = tile + EW_TILE * rs + EW_CH;
    double* muv = wv + EW_TILE;
    double* dinvH = muv + EW_TILE;
    double* dinvB = dinvH + rp;
    double* bet = dinvB + rp;

    const TaskView t = task_view(A.P, task);
    const int T = t.T, r = t.r, l = t.l;
    const int64_t r0 = t.r0;
    if (r < 1 || r > rp || T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        if (lane < 4) A.out[(int64_t)task * 4 + lane] = __builtin_nan("");
        if (lane == 0) A.flag[task] = 1;
        return;
    }
    const int j = lane < r ? lane : 0;  // the lane's column (lanes >= r compute on column 0 and store nothing)
    wave_zero(lds, 2 * rp * rs + EW_TILE * rs + EW_CH, lane);

    // ---- pass 1: G'WG, G'G, G'mu ----
    double cj = 0.0;
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
        if (lane < nt) {
            const int64_t at = (r0 + t0 + lane) * L + l;
            wv[lane] = A.w[at];
            muv[lane] = A.mu[at];
        }
        wave_sync();
        for (int tt = 0; tt < nt; ++tt) cj = fma(tile[tt * rs + j], muv[tt], cj);
        accum_gwg<true>(tile, wv, nt, r, rs, j, lane, Hm, Bm);
        wave_sync();  // (the tile is overwritten next)
    }
    if (lane < r) Hm[lane * rs + lane] += 1.0;
    wave_sync();

    // ---- factor both ----
    int bad = wave_chol(Hm, r, rs, dinvH, lane);
    bad |= wave_chol(Bm, r, rs, dinvB, lane);

    // log det H = 2 sum log L[k][k]
    const double logdet = 2.0 * wave_sum(lane < r ? log(Hm[lane * rs + lane]) : 0.0);

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
    const double trS = wave_sum(lane < r ? tr : 0.0);

    // beta = (G'G)^-1 G'mu
    const double z = wave_solve_llt(Bm, dinvB, r, rs, lane < r ? cj : 0.0, lane);
    const double bb = wave_sum(lane < r ? z * z : 0.0);
    if (lane < r) bet[lane] = z;
    wave_sync();

    // ---- pass 2: |mu - G beta|^2, lane tt one row of the tile ----
    double res = 0.0;
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
        wave_sync();
        if (lane < nt) {
            const double d = A.mu[(r0 + t0 + lane) * L + l] - tile_row_dot(tile + lane * rs, bet, r);
            res = fma(d, d, res);
        }
        wave_sync();
    }
    const double resid = wave_sum(res);
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
    R.m = fill_row_model(ctx, us, us, vb);
    R.n_blk = (int)((us.rows + 255) / 256);
    R.row_ell = d_row_ell;
    R.part = d_part;
    hipLaunchKernelGGL(elbo_rows, dim3((unsigned)R.n_blk), dim3(256), 0, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());
    CHK(launch_sums_finish(ctx, ctx->N, R.n_blk, d_part, d_sums));

    ElboKlArgs K;
    K.P = fill_task_prior(ctx, us);
    K.rp = rp;
    K.rs = rp | 1;
    K.mu = us.mu; K.w = us.w;
    K.out = d_terms; K.flag = d_flag;
    if (rp < 1 || rp > VLGP_WAVE) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_elbo: effective rank %d outside [1, %d]", rp, VLGP_WAVE);
    const size_t lds = sizeof(double) * (size_t)elbo_kl_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "vlgp_elbo: rank %d needs %zu bytes of LDS", rp, lds);
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)elbo_kl, ctx->lds_max));
    hipLaunchKernelGGL(elbo_kl, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
