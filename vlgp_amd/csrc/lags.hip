// Lag moments of the predictive distribution (vlgp_lag_moments): per replica three (K + 1, N) tables summed
// over the pairs of rows (t, t + k) of one unit,
//
//   resid[k, n] = sum d_tn d_{t+k,n}                           d = y - e, e the predictive mean of vlgp_pair_moments
//   model[k, n] = sum s_tn s_{t+k,n} f(q_n(t, t + k))          s = e, f = expm1 Poisson; s = 1, f = identity Gaussian
//   count[k, n] = the pairs in the sums;  model[0, n] += e_tn Poisson, noise_n Gaussian
//
// with q_n(t, s) = sum_l a_ln^2 c_l(t, s) and c_l the cross-time covariance of latent l under the mean-field posterior:
// H_l = I + G_l' diag(w_.l) G_l = Lc Lc', u_t = Lc^-1 G_l[t]', c_l(t, s) = u_t . u_s; w recomputed from mu, v over the
// entries the posterior saw.  A pair is in the sums when both entries are live (a select: y of an entry that is not live is
// never loaded) and every H_l of its unit has a factor.  Four kernels, fp64, no atomics, every sum in a fixed order:
//
// lag_rows     one lane per (row, replica): w_tl = sum_n seen a_ln^2 (rate Poisson, 1 / noise Gaussian), eight latents in
//              registers at a time (a set with more latents walks its channels once per eight).
// lag_task     one wave per (unit, latent) from the steps of eval_wave.h: G'WG over tiles of 64 rows, the Cholesky factor;
//              then tiles of 64 rows with the K rows behind them: every lane forward-substitutes its rows to u in place in
//              LDS (odd row stride) and writes c(t, t + k), k = 0 ... min(K, T - 1 - t), to the workspace (row, k, l).  The
//              halo rows of a tile are substituted again by the next tile: K / 64 of the substitutions twice, no ring.
// lag_moments  one wave per (row chunk, tile of 64 channels, replica), one lane per channel.  The wave walks its rows in
//              order; a lane keeps d, s and live of its channel's last K + 1 rows in a ring in LDS (nothing is shared
//              between lanes: no barrier) and adds, lag-outer, LAG_GROUP lags per walk in registers: the pairs (s - k, s)
//              whose earlier row is in the chunk and in the unit of s.  c(t, k, .) is read at wave-uniform addresses.
// lag_finish   adds the chunks in chunk order.
// vb == 0: c == 0, so only the last two run, compiled without the reads of c.
#include "call_block.h"
#include "eval_wave.h"
#include "fast_exp.h"

namespace {

#define LG_LCH 8  // latents of w a lane holds in registers at a time

struct LagRowArgs {
    RowModel m;
    const unsigned long long* mask;  // MASKED: (n_rep rows, nw), a set bit = held out = not seen
    int nw;
    double* w;                       // (n_rep rows, L)
};

template <bool MASKED>
__global__ void __launch_bounds__(256) lag_rows(LagRowArgs A) {
    const RowModel& M = A.m;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= M.rows) return;
    const int64_t mrow = (int64_t)blockIdx.y * M.rows + row;
    for (int l0 = 0; l0 < M.L; l0 += LG_LCH) {
        double acc[LG_LCH];
#pragma unroll
        for (int i = 0; i < LG_LCH; ++i) acc[i] = 0.0;
        for (int n = 0; n < M.N; ++n) {
            if (MASKED && ((A.mask[mrow * A.nw + (n >> 6)] >> (n & 63)) & 1ull)) continue;
            const double curv = M.gauss[n] ? 1.0 / M.noise[n]
                                           : exp(clamp10(row_eta(M, row, mrow, n) + row_quad(M, mrow, n, 0.0)));
#pragma unroll
            for (int i = 0; i < LG_LCH; ++i)
                if (l0 + i < M.L) {
                    const double al = M.a[(l0 + i) * M.N + n];
                    acc[i] = fma(al * al, curv, acc[i]);
                }
        }
#pragma unroll
        for (int i = 0; i < LG_LCH; ++i)
            if (l0 + i < M.L) A.w[mrow * M.L + l0 + i] = acc[i];
    }
}

struct LagTaskArgs {
    TaskPrior P;
    int rp, rs, K;         // rp: largest effective rank of the set's priors; rs: LDS row stride (odd, >= rp)
    const double* w;       // (rows, L)
    double* c;             // (rows, K + 1, L)
    int* flag;             // (M, L): 1 = a pivot was not positive and finite
};

__global__ void __launch_bounds__(64) lag_task(LagTaskArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, task = blockIdx.x;
    if (task >= A.P.M * A.P.L) return;
    const int rp = A.rp, rs = A.rs, L = A.P.L, K = A.K, K1 = K + 1;
    double* Hm = lds;
    double* U = Hm + rp * rs;  // pass 1: the tile of G; pass 2: u of 64 + K rows
    double* wv = U + (EW_TILE + K) * rs + EW_CH;
    double* dinv = wv + EW_TILE;

    const TaskView t = task_view(A.P, task);
    const int T = t.T, r = t.r, l = t.l;
    const double nan = __builtin_nan("");
    if (r < 1 || r > rp || T < 1) {  // (the host sized the LDS from the same ranks: never taken, never out of bounds)
        for (int i = lane; i < T; i += 64)
            for (int k = 0; k <= min(K, T - 1 - i); ++k) A.c[((t.r0 + i) * K1 + k) * L + l] = nan;
        if (lane == 0) A.flag[task] = 1;
        return;
    }

    // ---- pass 1: H = I + G'WG = Lc Lc' ----
    const int j = lane < r ? lane : 0;  // the lane's column (lanes >= r compute on column 0 and store nothing)
    wave_zero(lds, rp * rs + EW_TILE * rs + EW_CH, lane);
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, U, lane);
        if (lane < nt) wv[lane] = A.w[(t.r0 + t0 + lane) * L + l];
        wave_sync();
        accum_gwg<false>(U, wv, nt, r, rs, j, lane, Hm, nullptr);
        wave_sync();  // (the tile is overwritten next)
    }
    if (lane < r) Hm[lane * rs + lane] += 1.0;
    wave_sync();
    const int bad = wave_chol(Hm, r, rs, dinv, lane);
    if (lane == 0) A.flag[task] = bad ? 1 : 0;

    // ---- pass 2: u_t = Lc^-1 G[t]' of a tile and the K rows behind it, then c(t, t + k) = u_t . u_{t+k} ----
    for (int t0 = 0; t0 < T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, T - t0), nh = min(EW_TILE + K, T - t0);
        stage_rows(t.G, r, r, rs, t0, nh, U, lane);
        wave_sync();
        for (int row = lane; row < nh; row += 64) {  // in place: entry i is read before it is replaced
            double* xr = U + row * rs;
            for (int i = 0; i < r; ++i) {
                double s = xr[i];
                for (int q = 0; q < i; ++q) s = fma(-Hm[i * rs + q], xr[q], s);
                xr[i] = s * dinv[i];
            }
        }
        wave_sync();
        if (lane < nt) {
            const double* ur = U + lane * rs;
            const int kmax = min(K, T - 1 - (t0 + lane));
            double* out = A.c + ((t.r0 + t0 + lane) * K1) * L + l;
            for (int k = 0; k <= kmax; ++k) {
                const double* uk = ur + k * rs;
                double dot = 0.0;
                for (int q = 0; q < r; ++q) dot = fma(ur[q], uk[q], dot);
                out[(int64_t)k * L] = bad ? nan : dot;
            }
        }
        wave_sync();  // (the rows are overwritten next)
    }
}

struct LagMomArgs {
    RowModel m;            // y, xb of the source's rows; mu, v of the posterior's set
    const unsigned long long* mask;  // MASKED: (n_rep rows, nw), a set bit = held out = live
    int nw;
    int K, chunk_rows, n_chunks, tiles;
    int units;             // units per replica
    const int64_t* off;    // (n_rep units + 1): the posterior set's unit offsets, in its own rows
    const double* c;       // VB: (n_rep rows, K + 1, L)
    const int* flag;       // VB: (n_rep units, L)
    double* part;          // (n_rep, tiles, n_chunks, 3, K + 1, 64)
};

// every H_l of unit u has a factor (wave-uniform)
template <bool VB>
__device__ __forceinline__ bool unit_ok(const LagMomArgs& A, int u) {
    if (!VB) return true;
    int bad = 0;
    for (int l = 0; l < A.m.L; ++l) bad |= A.flag[(int64_t)u * A.m.L + l];
    return !bad;
}

// LDS: a^2 (L, 64) | d (K + 1, 64) | s (K + 1, 64) | live (K + 1, 64) int; column `lane` of each is the lane's own
template <bool MASKED, bool VB>
__global__ void __launch_bounds__(64) lag_moments(LagMomArgs A) {
    extern __shared__ __align__(16) double lds[];
    const RowModel& M = A.m;
    const int L = M.L, N = M.N, K = A.K, K1 = K + 1;
    double* asq = lds;
    double* dr = asq + L * 64;
    double* sr = dr + K1 * 64;
    int* lr = reinterpret_cast<int*>(sr + K1 * 64);
    const int lane = threadIdx.x, n = blockIdx.y * 64 + lane, rep = blockIdx.z;
    const bool in = n < N;
    for (int l = 0; l < L; ++l) {
        const double al = in ? M.a[l * N + n] : 0.0;
        asq[l * 64 + lane] = al * al;
    }
    const int gs = in ? M.gauss[n] : 0;
    const double noise = in ? M.noise[n] : 0.0;

    const int64_t base = (int64_t)rep * M.rows;  // first row of the replica in the posterior's set
    const int64_t r0 = (int64_t)blockIdx.x * A.chunk_rows;
    const int64_t r1 = r0 + A.chunk_rows < M.rows ? r0 + A.chunk_rows : M.rows;
    const int64_t s_end = r1 + K < M.rows ? r1 + K : M.rows;
    // the unit of the chunk's first row: the last u of the replica with off[u] <= base + r0
    int u_first = rep * A.units;
    for (int hi = u_first + A.units; hi - u_first > 1;) {
        const int mid = u_first + (hi - u_first) / 2;
        if (A.off[mid] <= base + r0) u_first = mid; else hi = mid;
    }
    double* out = A.part + (((int64_t)rep * A.tiles + blockIdx.y) * A.n_chunks + blockIdx.x) * 3 * K1 * 64 + lane;

    for (int k0 = 0; k0 < K1; k0 += LAG_GROUP) {
        double res[LAG_GROUP], mod[LAG_GROUP], cnt[LAG_GROUP];
#pragma unroll
        for (int j = 0; j < LAG_GROUP; ++j) res[j] = mod[j] = cnt[j] = 0.0;
        int u = u_first, head = 0;
        int64_t u_lo = A.off[u] - base, u_hi = A.off[u + 1] - base;  // the unit's rows, within the replica
        bool ok = unit_ok<VB>(A, u);
        for (int64_t s = r0; s < s_end; ++s) {
            while (s >= u_hi) {
                ++u;
                u_lo = u_hi;
                u_hi = A.off[u + 1] - base;
                ok = unit_ok<VB>(A, u);
            }
            const int64_t mrow = base + s;
            const bool live = ok && in && (!MASKED || ((A.mask[mrow * A.nw + (n >> 6)] >> (n & 63)) & 1ull));
            double d = 0.0, sc = 0.0, ex = 0.0;
            if (live) {
                const double eta = row_eta(M, s, mrow, n);
                const double e = gs ? eta : exp(clamp10(row_quad(M, mrow, n, eta)));
                d = M.y[s * N + n] - e;
                sc = gs ? 1.0 : e;
                ex = gs ? noise : e;
            }
            dr[head * 64 + lane] = d;
            sr[head * 64 + lane] = sc;
            lr[head * 64 + lane] = live ? 1 : 0;
            // the pairs (s - k, s): the earlier row in the chunk and in the unit of s
            const int64_t t_lo = r0 > u_lo ? r0 : u_lo;
            const int kmax = (int)(s - t_lo < K ? s - t_lo : K), kmin = (int)(s - (r1 - 1) > 0 ? s - (r1 - 1) : 0);
            if (ok) {
#pragma unroll
                for (int j = 0; j < LAG_GROUP; ++j) {
                    const int k = k0 + j;
                    if (k < kmin || k > kmax) continue;  // (wave-uniform)
                    const int slot = head - k < 0 ? head - k + K1 : head - k;
                    double q = 0.0;
                    if (VB) {
                        const double* cp = A.c + ((mrow - k) * K1 + k) * L;
                        for (int l = 0; l < L; ++l) q = fma(asq[l * 64 + lane], cp[l], q);
                    }
                    if (live && lr[slot * 64 + lane]) {
                        const double f = gs ? q : expm1(q);
                        res[j] = fma(dr[slot * 64 + lane], d, res[j]);
                        mod[j] += fma(sr[slot * 64 + lane] * sc, f, k == 0 ? ex : 0.0);
                        cnt[j] += 1.0;
                    }
                }
            }
            head = head + 1 == K1 ? 0 : head + 1;
        }
#pragma unroll
        for (int j = 0; j < LAG_GROUP; ++j)
            if (k0 + j < K1) {
                out[(int64_t)(0 * K1 + k0 + j) * 64] = res[j];
                out[(int64_t)(1 * K1 + k0 + j) * 64] = mod[j];
                out[(int64_t)(2 * K1 + k0 + j) * 64] = cnt[j];
            }
    }
}

// resid, model, count (n_rep, K + 1, N) = the partials of every (replica, tile, lag) added in chunk order.  Grid (K + 1,
// tiles, n_rep), 64 threads: one channel each.
__global__ void __launch_bounds__(64) lag_finish(const double* part, int N, int K1, int n_chunks, int tiles, double* resid,
                                                 double* model, double* count) {
    const int k = blockIdx.x, n = blockIdx.y * 64 + threadIdx.x;
    if (n >= N) return;
    const double* p = part + (((int64_t)blockIdx.z * tiles + blockIdx.y) * n_chunks) * 3 * K1 * 64 + (int64_t)k * 64 + threadIdx.x;
    double r = 0.0, m = 0.0, c = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch, p += (int64_t)3 * K1 * 64) {
        r += p[0];
        m += p[(int64_t)K1 * 64];
        c += p[(int64_t)2 * K1 * 64];
    }
    const int64_t at = ((int64_t)blockIdx.z * K1 + k) * N + n;
    resid[at] = r;
    model[at] = m;
    count[at] = c;
}

template <bool MASKED, bool VB>
int launch_moments(vlgp_ctx* ctx, const LagMomArgs& A, const dim3& grid, size_t lds) {
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)lag_moments<MASKED, VB>, ctx->lds_max));
    hipLaunchKernelGGL((lag_moments<MASKED, VB>), grid, dim3(64), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

}  // namespace

int launch_lag_moments(vlgp_ctx* ctx, UnitSet& us, int vb, int K, int rp, const LagLayout& o, double* d_w, double* d_c,
                       int* d_flag, double* d_part, double* d_resid, double* d_model, double* d_count) {
    static const char* who = "vlgp_lag_moments";
    const bool masked = us.is(SET_BY_ROW);
    const int n_rep = masked ? us.rep.n : 1;
    const RowModel M = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, vb);
    if (M.rows < 1 || us.M < 1 || us.M % n_rep) return vlgp_fail(ctx, VLGP_ERR_STATE, "%s on an empty set", who);
    if (o.n_chunks > 0x7fffffffLL || o.tiles > 65535 || n_rep > 65535 || (M.rows + 255) / 256 > 0x7fffffffLL)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: at most 65535 channel tiles and 65535 replicas per set", who);
    if (vb) {
        LagRowArgs R;
        R.m = M;
        R.mask = us.rep.d_mask;
        R.nw = us.rep.nw;
        R.w = d_w;
        const dim3 rgrid((unsigned)((M.rows + 255) / 256), (unsigned)n_rep);
        if (masked) hipLaunchKernelGGL(lag_rows<true>, rgrid, dim3(256), 0, ctx->stream, R);
        else hipLaunchKernelGGL(lag_rows<false>, rgrid, dim3(256), 0, ctx->stream, R);
        HIPCHK(ctx, hipGetLastError());

        LagTaskArgs T;
        T.P = fill_task_prior(ctx, us);
        T.rp = rp;
        T.rs = rp | 1;
        T.K = K;
        T.w = d_w;
        T.c = d_c;
        T.flag = d_flag;
        const size_t tlds = sizeof(double) * (size_t)lag_task_lds_doubles(T.rp, T.rs, K);
        if ((int64_t)tlds > ctx->lds_max)
            return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: rank %d at max_lag %d needs %zu bytes of LDS", who, rp, K, tlds);
        if (tlds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)lag_task, ctx->lds_max));
        hipLaunchKernelGGL(lag_task, dim3((unsigned)(us.M * ctx->L)), dim3(64), tlds, ctx->stream, T);
        HIPCHK(ctx, hipGetLastError());
    }
    LagMomArgs A;
    A.m = M;
    A.mask = us.rep.d_mask;
    A.nw = us.rep.nw;
    A.K = K;
    A.chunk_rows = (int)o.chunk_rows;
    A.n_chunks = (int)o.n_chunks;
    A.tiles = (int)o.tiles;
    A.units = us.M / n_rep;
    A.off = us.d_off;
    A.c = d_c;
    A.flag = d_flag;
    A.part = d_part;
    const size_t lds = (size_t)lag_moments_lds_bytes(ctx->L, K);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: %d latents need %zu bytes of LDS", who, ctx->L, lds);
    const dim3 grid((unsigned)o.n_chunks, (unsigned)o.tiles, (unsigned)n_rep);
    CHK((vb ? (masked ? launch_moments<true, true> : launch_moments<false, true>)
            : (masked ? launch_moments<true, false> : launch_moments<false, false>))(ctx, A, grid, lds));
    hipLaunchKernelGGL(lag_finish, dim3((unsigned)(K + 1), (unsigned)o.tiles, (unsigned)n_rep), dim3(64), 0, ctx->stream, d_part,
                       ctx->N, K + 1, A.n_chunks, A.tiles, d_resid, d_model, d_count);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
