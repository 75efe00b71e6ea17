// Joint Laplace posterior of a unit set (vlgp_joint_laplace): the mode of the posterior over ALL prior weights of a unit,
// found by a damped Newton iteration on the device, the Laplace evidence, latent variances that include the coupling
// between latents, and joint Gaussian draws for the importance weights of marginal.hip.  vlgp_joint_posterior is the same
// iteration without draws, also on a masked set of one replica, with the L x L covariance of the latents of every row,
// cov[t; l, l'] = G_l[t, :] (H^-1)_ll' G_l'[t, :]', in place of v.
//
// For one unit of T rows, G_l (T x r_l) the compact prior factor of latent l as task_view hands it out, the stacked index
// I = (l, i) latent-major, D = sum_l r_l <= 512 (vlgp_joint_laplace refuses more: the factor's panel must fit LDS):
//   x[t, l] = G_l[t, :] . beta_l,   eta[t, n] = a_n . x[t] + (b x)_tn                    (no v term: vlgp_marginal's ll)
//   Poisson   lam = exp(min(eta, 10)),  ll = y eta - lam - lgamma(y + 1),  res = y - lam,  cur = lam
//   Gaussian  ll = -log(2 pi noise_n) / 2 - (y - eta)^2 / (2 noise_n),  res = (y - eta) / noise_n,  cur = 1 / noise_n
//   f(beta) = 1/2 |beta|^2 - sum_t sum_n ll
//   grad_l f = beta_l - G_l' g[:, l],                    g[t, l] = sum_n a[l, n] res[t, n]
//   H[(l, i), (l', j)] = delta + sum_t G_l[t, i] c[t, l, l'] G_l'[t, j],   c[t, l, l'] = sum_n a[l, n] a[l', n] cur[t, n]
//   H = Lc Lc'
// Start: the mean-field centres m_l = H_l^-1 G_l'(g + w o mu)_l of task_weight_posterior (the caller's z, vb = 0); a
// masked set (vlgp_joint_posterior) starts at beta = 0: forecast_rows' z reads every y, and the mode does not depend on
// the start.
// Iteration, per unit: y = Lc^-1 grad f, decrement = |y|^2; stop (converged) when decrement <= tol, stop (not converged)
// after max_iter factorisations; else d = Lc^-T y and the trial point beta - s d, s = 1.  The trial is accepted when
//   f(beta - s d) <= f(beta) - JT_ARMIJO s decrement + JT_SLACK (1/2 |beta - s d|^2 + sum |ll terms of the rows|),
// the last term the rounding of the sum f is; otherwise s is halved and the NEXT row pass evaluates the shorter step against
// the same factor.  A step shorter than JT_MIN_STEP ends the unit where it stands (not converged).  f never increases
// beyond that rounding.  At the end: ll(beta), laplace = ll - 1/2 |beta|^2 - 1/2 log det H, mu[t, l] = x[t, l],
// v[t, l] = G_l[t, :] (H^-1)_ll G_l[t, :]', and for draw k: beta_k = beta + Lc^-T eps_k,
// c_k = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H; marginal_rows and marginal_finish turn beta_k, c_k into log_w.
//
// Kernels (DESIGN 4.11 has the reasons):
//   joint_init     one wave per (unit, latent): m_l into beta (marginal_task's first half).
//   joint_rows     one lane per row: x, the row's ll and sum |terms|, res and cur channel-major into a workspace, then g
//                  and the packed c from that workspace.  Rows of finished units are skipped.  joint_rows_masked is the
//                  same body (joint_row<MASKED>) with the mask words of the row, one replica, so the mask row is the
//                  row: a held-out entry adds nothing to ll and sum |terms|, its res = cur = 0, and y is not read there.
//   joint_decide   one workgroup per unit: f of the trial point, accept or halve.
//   joint_assemble one workgroup of 256 per (unit, pair of latents l' <= l): the r_l x r_l' block of H, rows of G_l o c and
//                  G_l' staged 32 at a time in LDS, a 4 x 4 register tile per thread.  H is a (D + 1) x (D + 1) row-major
//                  buffer per unit in global memory (L2): the strict lower triangle holds H, row D holds grad f.
//   joint_factor   one workgroup of 256 per unit: grad f into row D, then a left-looking Cholesky blocked by panels of
//                  JT_NB columns over rows 0 .. D: the panel's update against the finished columns in registers (one
//                  thread per row, JT_NB accumulators), the panel itself in LDS, one barrier per column.  The factor goes
//                  TRANSPOSED into the upper triangle and the diagonal (entry (q, i) = Lc[i, q]: threads of consecutive
//                  rows read consecutive addresses), so column D of the buffer ends as y = Lc^-1 grad f for free.  Then
//                  the decision above and, by one wave, the back substitution for d.
//   joint_var      one wave per (unit, latent): lane j the column (l, j) of H^-1 by two substitutions in a per-lane global
//                  vector, the r x r block (H^-1)_ll into LDS, then lane = row: v and mu.
//   joint_cov      vlgp_joint_posterior's joint_var, one wave per (unit, latent l): lane j the WHOLE column (l, j) of
//                  H^-1 -- the forward substitution still starts at the latent's first index, the back substitution runs
//                  down to index 0 -- in the same per-lane global vector; then for every l' <= l the r_l' x r_l block
//                  (H^-1)_l'l into LDS, and lane = row: cov[t; l, l'] = G_l'[t, :] (H^-1)_l'l G_l[t, :]' at pair
//                  l (l + 1) / 2 + l', summed as joint_var sums v (over i of G_l' in order, each term a chain over j), so
//                  the pair (l, l) is joint_var's v bit for bit; mu as there.
//   joint_stats    one workgroup per unit: the sums of the final row pass into stats.
//   joint_draw     one wave per unit, lane k one sample: the back substitution against Lc' in a per-lane global vector.
//   joint_window_moments      vlgp_joint_posterior_moments, after the finish: one workgroup of 256 per (unit, latent).  Wave 0
//                  solves for (H^-1)_ll as joint_var does, into LDS; then for every window of W <= 64 rows of the unit the
//                  rows of G_l go to LDS, Z = G_w (H^-1)_ll (W x r) is formed there, and Z G_w' + m_w m_w' is added to a
//                  4 x 4 register tile per thread of the unit's W x W sum (joint_assemble's tiling), which is kept across
//                  the windows.  Three tiles of 64 x 65 doubles and m_w: 100 352 bytes of LDS, above the 64 KB a kernel
//                  gets by default, so the launcher raises the ceiling as joint_factor's does.  A failed unit writes NaN.
//   joint_window_moments_sum  the (unit, latent) partials added over the units in unit order: S (L, W, W).
// A pivot that is not positive and finite marks the unit failed: its stats[0 .. 4], mu, v and c are NaN.  Every sum has a
// fixed order; the only atomic is the integer count of finished units.  Every index stays in bounds whatever the values.
#include <algorithm>

#include "eval_wave.h"
#include "fast_exp.h"

#define JT_NB 32                       // columns of a Cholesky panel
#define JT_PS (JT_NB + 1)              // LDS row stride of the panel
#define JT_ARMIJO 1e-4                 // sufficient decrease: fraction of the linear prediction s * decrement
#define JT_SLACK 0x1p-46               // rounding of f, relative to the sum of its absolute terms
#define JT_MIN_STEP 0x1p-30            // a step shorter than this ends the unit
#define JT_STATIC_LDS 1024             // room left for joint_factor's own __shared__ variables under the device's limit
#define JT_ST 8                        // per-unit state: doubles {s, f, decrement, log det H}, ints below
#define JW_N 64                        // joint_window_moments: the largest window and the largest rank
#define JW_LS (JW_N + 1)               // LDS row stride of its three tiles
enum { JI_DONE = 0, JI_NFACT, JI_CONV, JI_FAILED, JI_NEED };

namespace {

struct JointArgs {
    RowModel m;
    TaskPrior P;
    int R, Dmax, npair, max_iter, final;
    double tol;
    double* beta;      // (M, L, R), entries >= r_l zero
    double* dvec;      // (M, L, R) Newton direction, zero padded alike
    double* sd;        // (M, JT_ST)
    int* si;           // (M, JT_ST)
    int* n_done;
    double* x;         // (rows, L)
    double* llrow;     // (rows)
    double* absrow;    // (rows)
    double* g;         // (rows, L)
    double* c;         // (rows, npair), pair (l, l') at l (l + 1) / 2 + l'
    double* res;       // (N, rows)
    double* cur;       // (N, rows)
    double* H;         // (M, (Dmax + 1)^2)
    double* zw;        // (M * L, Dmax, 64) per-lane vectors of joint_var; joint_draw uses the first (M, Dmax, 64)
};

__device__ __forceinline__ int unit_rank(const TaskPrior& P, int p, int l, int R) {
    const int r = P.prior_rl[p * P.L + l];
    return (r < 1 || r > R || r > VLGP_WAVE) ? 0 : r;  // (the host refused such a set: never taken)
}

// doff[0 .. L]: first stacked index of each latent, doff[L] = D; by thread 0, behind a barrier
__device__ __forceinline__ void unit_offsets(const JointArgs& A, int p, int* doff) {
    if (threadIdx.x == 0) {
        int D = 0;
        for (int l = 0; l < A.P.L; ++l) {
            doff[l] = D;
            D += unit_rank(A.P, p, l, A.R);
        }
        doff[A.P.L] = D > A.Dmax ? 0 : D;  // (Dmax is the largest D of the set: never taken)
    }
    __syncthreads();
}

// three sums over a workgroup of 256 in a fixed order: a butterfly over each wave, then the four waves in order
__device__ __forceinline__ void block_sum3(double (&s)[3], double (*red)[3]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double t = wave_sum(s[j]);
        if (lane == 0) red[wid][j] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    __syncthreads();
}

// ---- start: the mean-field centres ----------------------------------------------------------------------------------
struct JointInitArgs {
    TaskPrior P;
    int R, rp, rs;
    const double* w;
    const double* z;
    double* beta;
    double* dvec;
};

__host__ __device__ inline int joint_wave_lds_doubles(int rp, int rs) {
    return rp * rs + EW_TILE * rs + EW_CH + 2 * EW_TILE + 2 * rp;  // marginal_task's: H | tile | w | z | 1/diag | spare
}

__global__ void __launch_bounds__(64) joint_init(JointInitArgs A) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, task = blockIdx.x;
    if (task >= A.P.M * A.P.L) return;
    const int rp = A.rp, rs = A.rs;
    double* Hm = lds;
    double* tile = Hm + rp * rs;
    double* wv = tile + EW_TILE * rs + EW_CH;
    double* zv = wv + EW_TILE;
    double* dinv = zv + EW_TILE;
    const TaskView t = task_view(A.P, task);
    double* bo = A.beta + (int64_t)task * A.R;
    double* dd = A.dvec + (int64_t)task * A.R;
    const double nan = __builtin_nan("");
    for (int i = lane; i < A.R; i += 64) bo[i] = dd[i] = 0.0;
    if (t.r < 1 || t.r > rp || t.r > A.R || t.T < 1) {  // (the host sized the LDS from the same ranks: never taken)
        if (lane == 0) bo[0] = nan;
        return;
    }
    int bad;
    const double mz = task_weight_posterior(t, A.P.L, A.w, A.z, rs, lane, lds, rp * rs + EW_TILE * rs + EW_CH, Hm, tile, wv,
                                            zv, dinv, &bad);
    if (lane < t.r) bo[lane] = bad ? nan : mz;  // (a NaN start makes every pivot of H NaN: the unit is counted as failed)
}

// ---- the row pass ---------------------------------------------------------------------------------------------------
template <bool MASKED>
__device__ __forceinline__ void joint_row(const JointArgs& A, const unsigned long long* mask, int nw) {
    const RowModel& M = A.m;
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= M.rows) return;
    const unsigned long long* mk = MASKED ? mask + row * nw : nullptr;  // (one replica: the row of the mask is the row)
    const int L = M.L, N = M.N;
    int u = 0;
    for (int hi = A.P.M; hi - u > 1;) {  // off[u] <= row < off[u + 1]
        const int mid = u + (hi - u) / 2;
        if (A.P.off[mid] <= row) u = mid; else hi = mid;
    }
    const int* si = A.si + (int64_t)u * JT_ST;
    if (!A.final && si[JI_DONE]) return;
    const bool trial = !A.final && si[JI_NFACT] > 0;
    const double s = A.sd[(int64_t)u * JT_ST];
    const int64_t t = row - A.P.off[u];
    const int p = A.P.unit_prior[u];
    for (int l = 0; l < L; ++l) {
        const int r = unit_rank(A.P, p, l, A.R);
        const double* __restrict__ G = A.P.prior_base[p] + A.P.prior_goff[p * L + l] + t * r;
        const double* __restrict__ b = A.beta + ((int64_t)u * L + l) * A.R;
        const double* __restrict__ d = A.dvec + ((int64_t)u * L + l) * A.R;
        double x = 0.0;
        for (int q = 0; q < r; ++q) x = fma(G[q], trial ? fma(-s, d[q], b[q]) : b[q], x);
        A.x[row * L + l] = x;
    }
    double ll = 0.0, ab = 0.0;
    for (int n = 0; n < N; ++n) {
        double eta = M.xb ? M.xb[row * N + n] : M.b[n];
        for (int l = 0; l < L; ++l) eta = fma(A.x[row * L + l], M.a[l * N + n], eta);
        if (MASKED && ((mk[n >> 6] >> (n & 63)) & 1ull)) {  // held out: no term, and y is not read
            A.res[(int64_t)n * M.rows + row] = 0.0;
            A.cur[(int64_t)n * M.rows + row] = 0.0;
            continue;
        }
        const double yv = M.y[row * N + n];
        double rs, cu;
        if (M.gauss[n]) {
            const double nz = M.noise[n], dd = yv - eta;
            const double k0 = 0.5 * log(2.0 * M_PI * nz), k1 = dd * dd / (2.0 * nz);
            ll -= k0 + k1;
            ab += fabs(k0) + k1;
            rs = dd / nz;
            cu = 1.0 / nz;
        } else {
            const double lam = exp(clamp10(eta)), lg = lgamma(yv + 1.0);
            ll += yv * eta - lam - lg;
            ab += fabs(yv * eta) + lam + lg;
            rs = yv - lam;
            cu = lam;
        }
        A.res[(int64_t)n * M.rows + row] = rs;
        A.cur[(int64_t)n * M.rows + row] = cu;
    }
    A.llrow[row] = ll;
    A.absrow[row] = ab;
    if (A.final) return;
    for (int l = 0; l < L; ++l) {
        double g = 0.0;
        for (int n = 0; n < N; ++n) g = fma(M.a[l * N + n], A.res[(int64_t)n * M.rows + row], g);
        A.g[row * L + l] = g;
        for (int l2 = 0; l2 <= l; ++l2) {
            double c = 0.0;
            for (int n = 0; n < N; ++n) c = fma(M.a[l * N + n] * M.a[l2 * N + n], A.cur[(int64_t)n * M.rows + row], c);
            A.c[row * A.npair + l * (l + 1) / 2 + l2] = c;
        }
    }
}

__global__ void __launch_bounds__(256) joint_rows(JointArgs A) { joint_row<false>(A, nullptr, 0); }
__global__ void __launch_bounds__(256) joint_rows_masked(JointArgs A, const unsigned long long* mask, int nw) {
    joint_row<true>(A, mask, nw);
}

// ---- accept or halve ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) joint_decide(JointArgs A) {
    __shared__ double red[4][3];
    __shared__ int verdict;
    const int u = blockIdx.x, tid = threadIdx.x;
    int* si = A.si + (int64_t)u * JT_ST;
    double* sd = A.sd + (int64_t)u * JT_ST;
    if (si[JI_DONE]) return;
    const bool trial = si[JI_NFACT] > 0;
    const double s = sd[0];
    const int64_t r0 = A.P.off[u];
    const int T = (int)(A.P.off[u + 1] - r0), LR = A.P.L * A.R;
    double* b = A.beta + (int64_t)u * LR;
    const double* d = A.dvec + (int64_t)u * LR;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < T; t += 256) {
        sum[0] += A.llrow[r0 + t];
        sum[1] += A.absrow[r0 + t];
    }
    for (int e = tid; e < LR; e += 256) {
        const double bt = trial ? fma(-s, d[e], b[e]) : b[e];
        sum[2] = fma(bt, bt, sum[2]);
    }
    block_sum3(sum, red);
    if (tid == 0) {
        const double f_trial = 0.5 * sum[2] - sum[0];
        bool accept = true;
        if (trial) accept = f_trial <= sd[1] - JT_ARMIJO * s * sd[2] + JT_SLACK * (0.5 * sum[2] + sum[1]);
        if (accept) {
            sd[1] = f_trial;
            si[JI_NEED] = 1;
        } else {
            sd[0] = 0.5 * s;
            si[JI_NEED] = 0;
            if (0.5 * s < JT_MIN_STEP) {
                si[JI_DONE] = 1;
                si[JI_CONV] = 0;
                atomicAdd(A.n_done, 1);
            }
        }
        verdict = accept ? 1 : 0;
    }
    __syncthreads();
    if (verdict && trial)
        for (int e = tid; e < LR; e += 256) b[e] = fma(-s, d[e], b[e]);
}

// ---- H, block by block ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) joint_assemble(JointArgs A) {
    __shared__ double As[32 * 64], Bs[32 * 64];
    __shared__ int doff[VLGP_MAX_L + 1];
    const int u = blockIdx.y, pair = blockIdx.x, tid = threadIdx.x, L = A.P.L;
    const int* si = A.si + (int64_t)u * JT_ST;
    if (si[JI_DONE] || !si[JI_NEED]) return;
    int l = 0;
    while ((l + 1) * (l + 2) / 2 <= pair) ++l;
    const int l2 = pair - l * (l + 1) / 2;
    const int p = A.P.unit_prior[u];
    unit_offsets(A, p, doff);
    const int D = doff[L], ld = D + 1;
    const int r = unit_rank(A.P, p, l, A.R), r2 = unit_rank(A.P, p, l2, A.R);
    if (D < 1 || r < 1 || r2 < 1) return;
    const int64_t r0 = A.P.off[u];
    const int T = (int)(A.P.off[u + 1] - r0);
    const double* __restrict__ G1 = A.P.prior_base[p] + A.P.prior_goff[p * L + l];
    const double* __restrict__ G2 = A.P.prior_base[p] + A.P.prior_goff[p * L + l2];
    const int i0 = (tid >> 4) * 4, j0 = (tid & 15) * 4;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int t0 = 0; t0 < T; t0 += 32) {
        for (int e = tid; e < 32 * 64; e += 256) {
            const int tt = e >> 6, i = e & 63, t = t0 + tt;
            const bool in = t < T;
            const double cv = in ? A.c[(r0 + t) * A.npair + pair] : 0.0;
            As[e] = (in && i < r) ? G1[(int64_t)t * r + i] * cv : 0.0;
            Bs[e] = (in && i < r2) ? G2[(int64_t)t * r2 + i] : 0.0;
        }
        __syncthreads();
        if (i0 < r && j0 < r2)
            for (int tt = 0; tt < 32; ++tt) {
                double a4[4], b4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a4[i] = As[tt * 64 + i0 + i];
                    b4[i] = Bs[tt * 64 + j0 + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fma(a4[i], b4[j], acc[i][j]);
            }
        __syncthreads();
    }
    double* buf = A.H + (int64_t)u * (A.Dmax + 1) * (A.Dmax + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int I = doff[l] + i0 + i, J = doff[l2] + j0 + j;
            if (i0 + i < r && j0 + j < r2 && J <= I) buf[(int64_t)I * ld + J] = acc[i][j] + (I == J ? 1.0 : 0.0);
        }
}

// ---- gradient, factor, decrement, direction -------------------------------------------------------------------------
__host__ __device__ inline int joint_factor_lds_doubles(int Dmax) { return (Dmax + 1) * JT_PS + JT_NB; }

__global__ void __launch_bounds__(256) joint_factor(JointArgs A) {
    extern __shared__ double lds[];  // the panel (D + 1 - k0 rows, stride JT_PS) | its diagonal (JT_NB)
    __shared__ int doff[VLGP_MAX_L + 1];
    __shared__ double red[4][3];
    __shared__ int go_on;
    const int u = blockIdx.x, tid = threadIdx.x, L = A.P.L;
    int* si = A.si + (int64_t)u * JT_ST;
    double* sd = A.sd + (int64_t)u * JT_ST;
    if (si[JI_DONE] || !si[JI_NEED]) return;
    const int p = A.P.unit_prior[u];
    unit_offsets(A, p, doff);
    const int D = doff[L], ld = D + 1;
    double* buf = A.H + (int64_t)u * (A.Dmax + 1) * (A.Dmax + 1);
    double* dg = lds + (A.Dmax + 1) * JT_PS;
    const int64_t r0 = A.P.off[u];
    const int T = (int)(A.P.off[u + 1] - r0);
    int bad = D < 1 ? 1 : 0;

    // grad f into row D
    for (int I = tid; I < D; I += 256) {
        int l = 0;
        while (doff[l + 1] <= I) ++l;
        const int i = I - doff[l], r = doff[l + 1] - doff[l];
        const double* __restrict__ G = A.P.prior_base[p] + A.P.prior_goff[p * L + l] + i;
        double s = 0.0;
        for (int t = 0; t < T; ++t) s = fma(G[(int64_t)t * r], A.g[(r0 + t) * L + l], s);
        buf[(int64_t)D * ld + I] = A.beta[((int64_t)u * L + l) * A.R + i] - s;
    }
    __syncthreads();

    double hl = 0.0;  // 1/2 log det H, the same in every thread
    for (int k0 = 0; k0 < D; k0 += JT_NB) {
        const int nb = min(JT_NB, D - k0), m = ld - k0;  // panel rows k0 .. D
        for (int ii = tid; ii < m; ii += 256) {
            const int i = k0 + ii;
            double acc[JT_NB];
#pragma unroll
            for (int j = 0; j < JT_NB; ++j) acc[j] = (j < nb && k0 + j <= i) ? buf[(int64_t)i * ld + k0 + j] : 0.0;
            for (int q = 0; q < k0; ++q) {
                const double* __restrict__ lq = buf + (int64_t)q * ld;
                const double li = lq[i];
#pragma unroll
                for (int j = 0; j < JT_NB; ++j) acc[j] = fma(-li, lq[min(k0 + j, D)], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < JT_NB; ++j) lds[ii * JT_PS + j] = acc[j];
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            double d = lds[j * JT_PS + j];
            for (int q = 0; q < j; ++q) d = fma(-lds[j * JT_PS + q], lds[j * JT_PS + q], d);
            bad |= (!(d > 0.0) || !(d < 1e300)) ? 1 : 0;
            const double sdv = sqrt(d);
            hl += log(sdv);
            if (tid == 0) dg[j] = sdv;
            for (int ii = j + 1 + tid; ii < m; ii += 256) {
                double s = lds[ii * JT_PS + j];
                for (int q = 0; q < j; ++q) s = fma(-lds[ii * JT_PS + q], lds[j * JT_PS + q], s);
                lds[ii * JT_PS + j] = s / sdv;
            }
            __syncthreads();
        }
        for (int j = 0; j < nb; ++j)
            for (int ii = j + tid; ii < m; ii += 256) buf[(int64_t)(k0 + j) * ld + k0 + ii] = ii == j ? dg[j] : lds[ii * JT_PS + j];
        __syncthreads();
    }

    double sum[3] = {0.0, 0.0, 0.0};
    for (int q = tid; q < D; q += 256) {
        const double yq = buf[(int64_t)q * ld + D];
        sum[0] = fma(yq, yq, sum[0]);
    }
    block_sum3(sum, red);
    const double dec = sum[0];
    if (tid == 0) {
        int done = 0;
        if (bad || !(dec == dec)) {
            si[JI_FAILED] = 1;
            done = 1;
        } else {
            sd[2] = dec;
            sd[3] = 2.0 * hl;
            si[JI_NFACT] += 1;
            if (dec <= A.tol) {
                si[JI_CONV] = 1;
                done = 1;
            } else if (si[JI_NFACT] >= A.max_iter) {
                done = 1;
            }
        }
        sd[0] = 1.0;
        si[JI_NEED] = 0;
        if (done) {
            si[JI_DONE] = 1;
            atomicAdd(A.n_done, 1);
        }
        go_on = !done;
    }
    __syncthreads();
    if (!go_on) return;

    // d = Lc^-T y by one wave, entry I after the entries behind it
    double* xs = lds;
    if (tid < 64) {
        for (int I = D - 1; I >= 0; --I) {
            const double* __restrict__ row = buf + (int64_t)I * ld;
            double s = 0.0;
            for (int Q = I + 1 + tid; Q < D; Q += 64) s = fma(row[Q], xs[Q], s);
            s = wave_sum(s);
            if (tid == 0) xs[I] = (row[D] - s) / row[I];
            wave_sync();
        }
    }
    __syncthreads();
    for (int I = tid; I < D; I += 256) {
        int l = 0;
        while (doff[l + 1] <= I) ++l;
        A.dvec[((int64_t)u * L + l) * A.R + I - doff[l]] = xs[I];
    }
}

// ---- variances ------------------------------------------------------------------------------------------------------
struct JointOutArgs {
    JointArgs J;
    int rp, rs, kc;
    double* stats;     // (M, 8)
    double* mu;        // (rows, L)
    double* v;         // (rows, L)
    const double* eps; // (M, L, R, 64)
    double* bk;        // (M, L, R, 64)
    double* ck;        // (M, L, 64)
};

__global__ void __launch_bounds__(64) joint_var(JointOutArgs O) {
    extern __shared__ double lds[];  // S (rp x rs) | tile (64 x rs)
    const JointArgs& A = O.J;
    const int lane = threadIdx.x, task = blockIdx.x, L = A.P.L;
    if (task >= A.P.M * L) return;
    const TaskView t = task_view(A.P, task);
    const int r = unit_rank(A.P, t.p, t.l, A.R);
    const int* si = A.si + (int64_t)t.u * JT_ST;
    int D = 0, d0 = 0;
    for (int l = 0; l < L; ++l) {
        if (l == t.l) d0 = D;
        D += unit_rank(A.P, t.p, l, A.R);
    }
    const double nan = __builtin_nan("");
    if (si[JI_FAILED] || r < 1 || r > O.rp || D > A.Dmax) {
        for (int tt = lane; tt < t.T; tt += 64) O.mu[(t.r0 + tt) * L + t.l] = O.v[(t.r0 + tt) * L + t.l] = nan;
        return;
    }
    const int ld = D + 1, rs = O.rs;
    const double* __restrict__ buf = A.H + (int64_t)t.u * (A.Dmax + 1) * (A.Dmax + 1);
    double* z = A.zw + (int64_t)task * A.Dmax * 64 + lane;  // entry I at z[I * 64]
    const int j = lane < r ? lane : 0;
    // y = Lc^-1 e_(d0 + j): zero above d0
    for (int I = d0; I < D; ++I) {
        double s = I == d0 + j ? 1.0 : 0.0;
        for (int Q = d0; Q < I; ++Q) s = fma(-buf[(int64_t)Q * ld + I], z[(int64_t)Q * 64], s);
        z[(int64_t)I * 64] = s / buf[(int64_t)I * ld + I];
    }
    // Lc^-T y, down to d0
    for (int I = D - 1; I >= d0; --I) {
        const double* __restrict__ row = buf + (int64_t)I * ld;
        double s = z[(int64_t)I * 64];
        for (int Q = I + 1; Q < D; ++Q) s = fma(-row[Q], z[(int64_t)Q * 64], s);
        z[(int64_t)I * 64] = s / row[I];
    }
    double* S = lds;
    double* tile = S + O.rp * rs;
    if (lane < r)
        for (int i = 0; i < r; ++i) S[i * rs + lane] = z[(int64_t)(d0 + i) * 64];
    wave_sync();
    for (int t0 = 0; t0 < t.T; t0 += EW_TILE) {
        const int nt = min(EW_TILE, t.T - t0);
        stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
        wave_sync();
        if (lane < nt) {
            const double* xr = tile + lane * rs;
            double var = 0.0;
            for (int i = 0; i < r; ++i) var = fma(xr[i], tile_row_dot(S + i * rs, xr, r), var);
            const int64_t at = (t.r0 + t0 + lane) * L + t.l;
            O.v[at] = var;
            O.mu[at] = A.x[at];
        }
        wave_sync();
    }
}

// joint_var with the cross blocks: cov (rows, npair), pair (l, l') at l (l + 1) / 2 + l'
__global__ void __launch_bounds__(64) joint_cov(JointOutArgs O, double* cov) {
    extern __shared__ double lds[];  // S (rp x rs) | tile of G_l (64 x rs) | tile of G_l' (64 x rs)
    const JointArgs& A = O.J;
    const int lane = threadIdx.x, task = blockIdx.x, L = A.P.L;
    if (task >= A.P.M * L) return;
    const TaskView t = task_view(A.P, task);
    const int r = unit_rank(A.P, t.p, t.l, A.R);
    const int* si = A.si + (int64_t)t.u * JT_ST;
    int D = 0, d0 = 0, rmax = 0;
    for (int l = 0; l < L; ++l) {
        if (l == t.l) d0 = D;
        const int rl = unit_rank(A.P, t.p, l, A.R);
        rmax = max(rmax, rl);
        D += rl;
    }
    const double nan = __builtin_nan("");
    const int pair0 = t.l * (t.l + 1) / 2;
    if (si[JI_FAILED] || r < 1 || rmax > O.rp || D > A.Dmax) {
        for (int tt = lane; tt < t.T; tt += 64) {
            O.mu[(t.r0 + tt) * L + t.l] = nan;
            for (int l2 = 0; l2 <= t.l; ++l2) cov[(t.r0 + tt) * A.npair + pair0 + l2] = nan;
        }
        return;
    }
    const int ld = D + 1, rs = O.rs;
    const double* __restrict__ buf = A.H + (int64_t)t.u * (A.Dmax + 1) * (A.Dmax + 1);
    double* z = A.zw + (int64_t)task * A.Dmax * 64 + lane;  // entry I at z[I * 64]
    const int j = lane < r ? lane : 0;
    // y = Lc^-1 e_(d0 + j): zero above d0
    for (int I = d0; I < D; ++I) {
        double s = I == d0 + j ? 1.0 : 0.0;
        for (int Q = d0; Q < I; ++Q) s = fma(-buf[(int64_t)Q * ld + I], z[(int64_t)Q * 64], s);
        z[(int64_t)I * 64] = s / buf[(int64_t)I * ld + I];
    }
    // Lc^-T y, down to 0: the whole column (the entries at and behind d0 are joint_var's)
    for (int I = D - 1; I >= 0; --I) {
        const double* __restrict__ row = buf + (int64_t)I * ld;
        double s = I >= d0 ? z[(int64_t)I * 64] : 0.0;  // (y is zero above d0 and was not stored there)
        for (int Q = I + 1; Q < D; ++Q) s = fma(-row[Q], z[(int64_t)Q * 64], s);
        z[(int64_t)I * 64] = s / row[I];
    }
    double* S = lds;
    double* tile = S + O.rp * rs;
    double* tile2 = tile + EW_TILE * rs;
    int d2 = 0;
    for (int l2 = 0; l2 <= t.l; ++l2) {
        const int r2 = unit_rank(A.P, t.p, l2, A.R);
        const double* __restrict__ G2 = A.P.prior_base[t.p] + A.P.prior_goff[t.p * L + l2];
        if (lane < r)
            for (int i = 0; i < r2; ++i) S[i * rs + lane] = z[(int64_t)(d2 + i) * 64];  // (H^-1)[(l2, i), (l, lane)]
        wave_sync();
        for (int t0 = 0; t0 < t.T; t0 += EW_TILE) {
            const int nt = min(EW_TILE, t.T - t0);
            stage_rows(t.G, r, r, rs, t0, nt, tile, lane);
            stage_rows(G2, r2, r2, rs, t0, nt, tile2, lane);
            wave_sync();
            if (lane < nt) {
                const double* xr = tile + lane * rs;
                const double* x2 = tile2 + lane * rs;
                double cv = 0.0;
                for (int i = 0; i < r2; ++i) cv = fma(x2[i], tile_row_dot(S + i * rs, xr, r), cv);
                cov[(t.r0 + t0 + lane) * A.npair + pair0 + l2] = cv;
                if (l2 == t.l) {
                    const int64_t at = (t.r0 + t0 + lane) * L + t.l;
                    O.mu[at] = A.x[at];
                }
            }
            wave_sync();  // (the tiles and S are overwritten next)
        }
        d2 += r2;
    }
}

__global__ void __launch_bounds__(256) joint_stats(JointOutArgs O) {
    __shared__ double red[4][3];
    const JointArgs& A = O.J;
    const int u = blockIdx.x, tid = threadIdx.x, L = A.P.L;
    const int64_t r0 = A.P.off[u];
    const int T = (int)(A.P.off[u + 1] - r0), LR = L * A.R;
    const double* b = A.beta + (int64_t)u * LR;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < T; t += 256) sum[0] += A.llrow[r0 + t];
    for (int e = tid; e < LR; e += 256) sum[2] = fma(b[e], b[e], sum[2]);
    block_sum3(sum, red);
    if (tid == 0) {
        const int* si = A.si + (int64_t)u * JT_ST;
        const double* sd = A.sd + (int64_t)u * JT_ST;
        const int p = A.P.unit_prior[u];
        int D = 0;
        for (int l = 0; l < L; ++l) D += unit_rank(A.P, p, l, A.R);
        double* st = O.stats + (int64_t)u * 8;
        const bool bad = si[JI_FAILED] != 0;
        const double nan = __builtin_nan("");
        st[0] = bad ? nan : (sum[0] - 0.5 * sum[2]) - 0.5 * sd[3];
        st[1] = bad ? nan : sum[0];
        st[2] = bad ? nan : sum[2];
        st[3] = bad ? nan : sd[3];
        st[4] = bad ? nan : sd[2];
        st[5] = (double)si[JI_NFACT];
        st[6] = (double)si[JI_CONV];
        st[7] = (double)D;
    }
}

// ---- draws ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) joint_draw(JointOutArgs O) {
    __shared__ int doff[VLGP_MAX_L + 1];
    const JointArgs& A = O.J;
    const int u = blockIdx.x, lane = threadIdx.x, L = A.P.L;
    const int p = A.P.unit_prior[u];
    unit_offsets(A, p, doff);
    const int D = doff[L], ld = D + 1;
    const bool live = lane < O.kc;
    const int k = live ? lane : 0;  // (a lane past kc works on sample 0 and stores nothing)
    const int* si = A.si + (int64_t)u * JT_ST;
    const double nan = __builtin_nan("");
    double* ck = O.ck + (int64_t)u * L * 64 + lane;
    if (live)
        for (int l = 1; l < L; ++l) ck[(int64_t)l * 64] = 0.0;
    if (si[JI_FAILED] || D < 1) {
        if (live) ck[0] = nan;
        return;
    }
    const double* __restrict__ buf = A.H + (int64_t)u * (A.Dmax + 1) * (A.Dmax + 1);
    double* xw = A.zw + (int64_t)u * A.Dmax * 64 + lane;
    const double* __restrict__ ek = O.eps + (int64_t)u * L * A.R * 64 + k;
    double e2 = 0.0;
    int l = L - 1;
    for (int I = D - 1; I >= 0; --I) {  // Lc^-T eps, entry I after the entries behind it
        while (doff[l] > I) --l;
        const double e = ek[((int64_t)l * A.R + I - doff[l]) * 64];
        e2 = fma(e, e, e2);
        const double* __restrict__ row = buf + (int64_t)I * ld;
        double s = e;
        for (int Q = I + 1; Q < D; ++Q) s = fma(-row[Q], xw[(int64_t)Q * 64], s);
        xw[(int64_t)I * 64] = s / row[I];
    }
    double b2 = 0.0;
    const double* b = A.beta + (int64_t)u * L * A.R;
    double* bk = O.bk + (int64_t)u * L * A.R * 64 + k;
    for (l = 0; l < L; ++l)
        for (int i = 0; i < doff[l + 1] - doff[l]; ++i) {
            const double bt = b[l * A.R + i] + xw[(int64_t)(doff[l] + i) * 64];
            b2 = fma(bt, bt, b2);
            if (live) bk[((int64_t)l * A.R + i) * 64] = bt;
        }
    if (live) ck[0] = (0.5 * e2 - 0.5 * b2) - 0.5 * A.sd[(int64_t)u * JT_ST + 3];
}

// ---- window moments of the hyperparameter step ----------------------------------------------------------------------
// part (M, L, W, W): for (unit, latent) the sum over the unit's windows of m_w m_w' + G_w (H^-1)_ll G_w', G_w = G_l[s : s + W]
// and m_w = x[s : s + W, l] of the final row pass; the starts are s = k W, k < T / W, and T - W when W does not divide T.
// Only the 4 x 4 tiles at or below the diagonal are summed and every entry above it is the copy of its mirror image.
__global__ void __launch_bounds__(256) joint_window_moments(JointOutArgs O, int W, double* part) {
    extern __shared__ double lds[];  // S | the window of G_l | Z = G_w S (64 x JW_LS each) | m_w (64)
    const JointArgs& A = O.J;
    const int tid = threadIdx.x, task = blockIdx.x, L = A.P.L;
    if (task >= A.P.M * L || W < 2 || W > JW_N) return;
    const TaskView t = task_view(A.P, task);
    const int r = unit_rank(A.P, t.p, t.l, A.R);
    const int* si = A.si + (int64_t)t.u * JT_ST;
    int D = 0, d0 = 0;
    for (int l = 0; l < L; ++l) {
        if (l == t.l) d0 = D;
        D += unit_rank(A.P, t.p, l, A.R);
    }
    double* out = part + (int64_t)task * W * W;
    if (si[JI_FAILED] || r < 1 || D > A.Dmax) {
        const double nan = __builtin_nan("");
        for (int e = tid; e < W * W; e += 256) out[e] = nan;
        return;
    }
    double* S = lds;
    double* Gw = S + JW_N * JW_LS;
    double* Z = Gw + JW_N * JW_LS;
    double* mw = Z + JW_N * JW_LS;
    for (int e = tid; e < JW_N * JW_LS; e += 256) S[e] = 0.0;
    __syncthreads();
    if (tid < r && t.T >= W) {  // joint_var's two substitutions: lane j the column (l, j) of H^-1 from d0 down
        const int ld = D + 1;
        const double* __restrict__ buf = A.H + (int64_t)t.u * (A.Dmax + 1) * (A.Dmax + 1);
        double* z = A.zw + (int64_t)task * A.Dmax * 64 + tid;  // entry I at z[I * 64]
        for (int I = d0; I < D; ++I) {
            double s = I == d0 + tid ? 1.0 : 0.0;
            for (int Q = d0; Q < I; ++Q) s = fma(-buf[(int64_t)Q * ld + I], z[(int64_t)Q * 64], s);
            z[(int64_t)I * 64] = s / buf[(int64_t)I * ld + I];
        }
        for (int I = D - 1; I >= d0; --I) {
            const double* __restrict__ row = buf + (int64_t)I * ld;
            double s = z[(int64_t)I * 64];
            for (int Q = I + 1; Q < D; ++Q) s = fma(-row[Q], z[(int64_t)Q * 64], s);
            z[(int64_t)I * 64] = s / row[I];
        }
        for (int i = 0; i < r; ++i) S[i * JW_LS + tid] = z[(int64_t)(d0 + i) * 64];
    }
    const int i0 = (tid >> 4) * 4, j0 = (tid & 15) * 4;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    const int nfull = t.T / W, nwin = t.T < W ? 0 : nfull + (t.T % W ? 1 : 0);
    for (int k = 0; k < nwin; ++k) {
        const int s0 = k < nfull ? k * W : t.T - W;
        __syncthreads();  // (S is whole; the last window's tiles are read)
        for (int e = tid; e < JW_N * JW_N; e += 256) {
            const int tt = e >> 6, i = e & 63;
            Gw[tt * JW_LS + i] = (tt < W && i < r) ? t.G[(int64_t)(s0 + tt) * r + i] : 0.0;
        }
        if (tid < JW_N) mw[tid] = tid < W ? A.x[(t.r0 + s0 + tid) * L + t.l] : 0.0;
        __syncthreads();
        if (i0 < W && j0 < r) {  // Z = G_w S
            double zt[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) zt[i][j] = 0.0;
            for (int q = 0; q < r; ++q) {
                double a4[4], b4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a4[i] = Gw[(i0 + i) * JW_LS + q];
                    b4[i] = S[q * JW_LS + j0 + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) zt[i][j] = fma(a4[i], b4[j], zt[i][j]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) Z[(i0 + i) * JW_LS + j0 + j] = zt[i][j];
        }
        __syncthreads();
        if (i0 < W && j0 <= i0) {  // += Z G_w' + m_w m_w'
            for (int q = 0; q < r; ++q) {
                double a4[4], b4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a4[i] = Z[(i0 + i) * JW_LS + q];
                    b4[i] = Gw[(j0 + i) * JW_LS + q];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fma(a4[i], b4[j], acc[i][j]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(mw[i0 + i], mw[j0 + j], acc[i][j]);
        }
    }
    if (j0 <= i0)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int I = i0 + i, J = j0 + j;
                if (I < W && J <= I) {
                    out[I * W + J] = acc[i][j];
                    out[J * W + I] = acc[i][j];
                }
            }
}

// S (L, W, W) = the partials of the units added in unit order
__global__ void __launch_bounds__(256) joint_window_moments_sum(int M, int L, int W2, const double* part, double* S) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)L * W2) return;
    const int l = (int)(e / W2), at = (int)(e % W2);
    double s = 0.0;
    for (int u = 0; u < M; ++u) s += part[((int64_t)u * L + l) * W2 + at];
    S[e] = s;
}

JointArgs fill_joint(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int max_iter, double tol, int final) {
    JointArgs A;
    A.m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, 0);  // (a masked set of one replica: the source's y, xb)
    A.P = fill_task_prior(ctx, us);
    A.R = ctx->R; A.Dmax = W.Dmax; A.npair = ctx->L * (ctx->L + 1) / 2; A.max_iter = max_iter; A.final = final;
    A.tol = tol;
    A.beta = W.beta; A.dvec = W.dvec; A.sd = W.sd; A.si = W.si; A.n_done = W.n_done;
    A.x = W.x; A.llrow = W.llrow; A.absrow = W.absrow; A.g = W.g; A.c = W.c; A.res = W.res; A.cur = W.cur;
    A.H = W.H; A.zw = W.zw;
    return A;
}

}  // namespace

int64_t joint_work_doubles(const vlgp_ctx* ctx, const UnitSet& us, int Dmax, JointWork* W) {
    const int64_t L = ctx->L, N = ctx->N, R = ctx->R, M = us.M, rows = us.rows, npair = L * (L + 1) / 2;
    int64_t o = 0;
    auto take = [&o](int64_t n) { const int64_t at = o; o += (n + 1) & ~(int64_t)1; return at; };
    const int64_t o_beta = take(M * L * R), o_d = take(M * L * R), o_sd = take(M * JT_ST), o_si = take(M * JT_ST / 2 + 1);
    const int64_t o_nd = take(2), o_x = take(rows * L), o_ll = take(rows), o_ab = take(rows), o_g = take(rows * L);
    const int64_t o_c = take(rows * npair), o_res = take(N * rows), o_cur = take(N * rows);
    const int64_t o_H = take(M * (int64_t)(Dmax + 1) * (Dmax + 1)), o_zw = take(M * L * (int64_t)Dmax * 64);
    if (W) {
        double* d = W->base;
        W->Dmax = Dmax;
        W->beta = d + o_beta; W->dvec = d + o_d; W->sd = d + o_sd; W->si = reinterpret_cast<int*>(d + o_si);
        W->n_done = reinterpret_cast<int*>(d + o_nd);
        W->x = d + o_x; W->llrow = d + o_ll; W->absrow = d + o_ab; W->g = d + o_g; W->c = d + o_c; W->res = d + o_res;
        W->cur = d + o_cur; W->H = d + o_H; W->zw = d + o_zw;
        W->state_bytes = sizeof(double) * (size_t)(o_x - o_sd);
    }
    return o;
}

// the start: z = g + w o mu (vb = 0) into W.g, the mean-field centres into W.beta, the per-unit state zeroed; a masked
// set starts at beta = 0
int launch_joint_init(vlgp_ctx* ctx, UnitSet& us, int rp, const JointWork& W) {
    if (rp < 1 || rp > VLGP_WAVE || rp > ctx->R)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: effective rank %d outside [1, %d]", W.who, rp, std::min(VLGP_WAVE, ctx->R));
    HIPCHK(ctx, hipMemsetAsync(W.sd, 0, W.state_bytes, ctx->stream));  // sd | si | n_done
    if (us.is(SET_BY_ROW)) {
        HIPCHK(ctx, hipMemsetAsync(W.beta, 0, sizeof(double) * (size_t)(W.sd - W.beta), ctx->stream));  // beta | dvec
        return VLGP_OK;
    }
    CHK(launch_forecast_z(ctx, us, 0, W.g));
    JointInitArgs K;
    K.P = fill_task_prior(ctx, us);
    K.R = ctx->R; K.rp = rp; K.rs = rp | 1;
    K.w = us.w; K.z = W.g; K.beta = W.beta; K.dvec = W.dvec;
    const size_t lds = sizeof(double) * (size_t)joint_wave_lds_doubles(K.rp, K.rs);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: rank %d needs %zu bytes of LDS", W.who, rp, lds);
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)joint_init, ctx->lds_max));
    hipLaunchKernelGGL(joint_init, dim3((unsigned)(us.M * ctx->L)), dim3(64), lds, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// the row pass of a plain set or of a masked set of one replica
static int launch_joint_rows(vlgp_ctx* ctx, UnitSet& us, const JointArgs& A) {
    const dim3 grid((unsigned)((us.rows + 255) / 256));
    if (us.is(SET_BY_ROW)) hipLaunchKernelGGL(joint_rows_masked, grid, dim3(256), 0, ctx->stream, A, us.rep.d_mask, us.rep.nw);
    else hipLaunchKernelGGL(joint_rows, grid, dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// one round: the row pass at every unfinished unit's trial point, accept or halve, and for the accepted ones H, its factor,
// the decrement and the next direction.  W.n_done counts the finished units.
int launch_joint_round(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int max_iter, double tol) {
    const JointArgs A = fill_joint(ctx, us, W, max_iter, tol, 0);
    const size_t lds = sizeof(double) * (size_t)joint_factor_lds_doubles(W.Dmax);
    const int ceiling = ctx->lds_max - JT_STATIC_LDS;  // (the kernel's own __shared__ variables count against the same limit)
    if ((int64_t)lds > ceiling) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: D = %d needs %zu bytes of LDS", W.who, W.Dmax, lds);
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)joint_factor, ceiling));
    CHK(launch_joint_rows(ctx, us, A));
    hipLaunchKernelGGL(joint_decide, dim3((unsigned)us.M), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(joint_assemble, dim3((unsigned)A.npair, (unsigned)us.M), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(joint_factor, dim3((unsigned)us.M), dim3(256), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// after the last round: the row pass at beta itself, then stats (M, 8) and, where asked for, mu (rows, L) with either v
// (rows, L: joint_var) or cov (rows, L (L + 1) / 2: joint_cov)
int launch_joint_finish(vlgp_ctx* ctx, UnitSet& us, int rp, const JointWork& W, double* d_stats, double* d_mu, double* d_v,
                        double* d_cov) {
    JointOutArgs O = {};
    O.J = fill_joint(ctx, us, W, 1, 0.0, 1);
    O.rp = rp; O.rs = rp | 1;
    O.stats = d_stats; O.mu = d_mu; O.v = d_v;
    CHK(launch_joint_rows(ctx, us, O.J));
    hipLaunchKernelGGL(joint_stats, dim3((unsigned)us.M), dim3(256), 0, ctx->stream, O);
    HIPCHK(ctx, hipGetLastError());
    if (d_mu && (d_v || d_cov)) {
        const size_t lds = sizeof(double) * (size_t)(O.rp * O.rs + (d_cov ? 2 : 1) * EW_TILE * O.rs);
        const void* fn = d_cov ? (const void*)joint_cov : (const void*)joint_var;
        if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: rank %d needs %zu bytes of LDS", W.who, rp, lds);
        if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, fn, ctx->lds_max));
        const dim3 grid((unsigned)(us.M * ctx->L));
        if (d_cov) hipLaunchKernelGGL(joint_cov, grid, dim3(64), lds, ctx->stream, O, d_cov);
        else hipLaunchKernelGGL(joint_var, grid, dim3(64), lds, ctx->stream, O);
        HIPCHK(ctx, hipGetLastError());
    }
    return VLGP_OK;
}

// after launch_joint_finish (the factor and x of the final row pass are in W): d_part (M, L, window, window) per (unit,
// latent), d_S (L, window, window) their sum over the units; 2 <= window <= 64 and rp <= 64: the caller has checked
int launch_joint_window_moments(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int window, double* d_part, double* d_S) {
    JointOutArgs O = {};
    O.J = fill_joint(ctx, us, W, 1, 0.0, 1);
    const size_t lds = sizeof(double) * (size_t)(3 * JW_N * JW_LS + JW_N);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: the window moments need %zu bytes of LDS", W.who, lds);
    CHK(vlgp_raise_lds(ctx, (const void*)joint_window_moments, (int)lds));
    hipLaunchKernelGGL(joint_window_moments, dim3((unsigned)(us.M * ctx->L)), dim3(256), lds, ctx->stream, O, window, d_part);
    HIPCHK(ctx, hipGetLastError());
    const int64_t n = (int64_t)ctx->L * window * window;
    hipLaunchKernelGGL(joint_window_moments_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, us.M, ctx->L,
                       window * window, d_part, d_S);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// kc <= 64 draws beta + Lc^-T eps into d_beta (M, L, R, 64) and their c into slot 0 of d_c (M, L, 64), the other slots
// zero: what launch_marginal_rows reads
int launch_joint_draw(vlgp_ctx* ctx, UnitSet& us, const JointWork& W, int kc, const double* d_eps, double* d_beta, double* d_c) {
    JointOutArgs O = {};
    O.J = fill_joint(ctx, us, W, 1, 0.0, 1);
    O.kc = kc; O.eps = d_eps; O.bk = d_beta; O.ck = d_c;
    hipLaunchKernelGGL(joint_draw, dim3((unsigned)us.M), dim3(64), 0, ctx->stream, O);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
