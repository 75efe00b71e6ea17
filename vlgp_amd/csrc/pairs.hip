// Pair moments of the predictive distribution (vlgp_pair_moments, vlgp_pair_moments_cov): per replica two
// N x N matrices summed over the rows,
//
//   resid[n, m] = sum_t live_tn live_tm d_tn d_tm          d = y - e, e the predictive mean
//   model[n, m] = sum_t live_tn live_tm K_t[n, m]          K_t the predictive covariance of the row
//
// under a Gaussian posterior N(mu_t, C_t) of the latents of every row: C_t = diag(v_t) (the set's own mu, v; 0 when
// vb == 0) or a supplied packed L x L covariance.  With c[n, m] = a_n' C_t a_m, u_m = C_t a_m:
//
//   m_n = a_n . mu_t + (b x)_tn                            row_eta's chain
//   e_n = trunc_exp(m_n + c[n, n] / 2) Poisson, m_n Gaussian   the rate of vlgp_predictive / vlgp_predictive_cov, their chains
//   s_n = e_n Poisson, 1 Gaussian
//   K[n, m] = s_n s_m f(c[n, m]),  f = expm1 when both channels are Poisson, else the identity;
//   K[n, n] += e_n Poisson, noise_n Gaussian
//
// The grid is (row chunk, channel-tile pair I >= J, replica), 256 threads, a 64 x 64 tile of pairs with a 4 x 4 register
// tile per thread for each sum; thread (ty, tx) owns the channels I 64 + ty + 16 i and J 64 + tx + 16 j, so a half wave
// reads 16 consecutive doubles of the J side and broadcasts the I side.  The workgroup walks the rows of its chunk: the
// row's mu and v or cov go to LDS once (a supplied row with a non-finite value is dead: skipped by every thread), 128
// threads stage d, s of the channels of both tiles and u of tile J, then every thread adds its 16 pairs.  `live` enters
// as d = s = 0 by a select: what y holds at an entry that is not live is never multiplied.  One partial per (chunk, tile
// pair, replica); pair_finish adds the chunks in chunk order and writes the upper triangle as the copy of the lower one:
// no atomics, the same bits on every run, both matrices symmetric to the bit.
#include "call_block.h"
#include "eval_wave.h"
#include "fast_exp.h"

namespace {

struct PairArgs {
    RowModel m;            // y, xb of the source's rows; mu, v of the posterior's set (mu: the supplied one under COV)
    const double* cov;     // COV: (rows of the posterior's set, L (L + 1) / 2)
    const unsigned long long* mask;  // MASKED: (n_rep rows, nw)
    int nw;
    int chunk_rows, n_chunks, tile_pairs;
    double* part;          // (n_rep, tile_pairs, n_chunks, 2, 64, 64)
};

// the tile pair p = I (I + 1) / 2 + J, J <= I
__device__ __forceinline__ void pair_tiles(int p, int* I, int* J) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    *I = i;
    *J = p - i * (i + 1) / 2;
}

// LDS, in doubles: aI (L, 64) | aJ (L, 64) | uJ (L, 64) | mc (L + max(L, L (L + 1) / 2)) | d (128) | s (128) | ex (64)
template <bool COV, bool MASKED>
__global__ void __launch_bounds__(256) pair_moments(PairArgs A) {
    extern __shared__ __align__(16) double lds[];
    const RowModel& M = A.m;
    const int L = M.L, N = M.N, npair = L * (L + 1) / 2;
    const int n_mc = L + (COV ? npair : L);
    double* aI = lds;
    double* aJ = aI + L * 64;
    double* uJ = aJ + L * 64;
    double* mc = uJ + L * 64;
    double* dv = mc + L + (npair > L ? npair : L);
    double* sv = dv + 128;
    double* ex = sv + 128;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int I, J;
    pair_tiles(blockIdx.y, &I, &J);
    const int k = blockIdx.z;

    // the loadings of both tiles, once; a channel past N loads zeros
    for (int e = tid; e < 2 * L * 64; e += 256) {
        const int side = e / (L * 64), r = e - side * L * 64, l = r >> 6, c = r & 63;
        const int n = (side ? J : I) * 64 + c;
        (side ? aJ : aI)[r] = n < N ? M.a[l * N + n] : 0.0;
    }
    // which of the thread's pairs are Poisson-Poisson: bit 4 i + j
    unsigned pp = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = I * 64 + ty + 16 * i, gj = J * 64 + tx + 16 * j;
            if (gi < N && gj < N && !M.gauss[gi] && !M.gauss[gj]) pp |= 1u << (4 * i + j);
        }
    // the channel this thread stages (threads 0 ... 127): side 0 tile I, side 1 tile J
    const int sc = tid & 63, side = (tid >> 6) & 1;
    const int sn = (side ? J : I) * 64 + sc;
    const bool stager = tid < 128 && sn < N;
    const double* sa = side ? aJ : aI;
    const int sgauss = stager ? M.gauss[sn] : 0;
    const double snoise = stager ? M.noise[sn] : 0.0;
    if (tid < 128 && !stager) {  // a channel past N: never live
        dv[tid] = sv[tid] = 0.0;
        if (side == 0) ex[sc] = 0.0;
        else for (int l = 0; l < L; ++l) uJ[l * 64 + sc] = 0.0;
    }

    double res[4][4], mod[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) res[i][j] = mod[i][j] = 0.0;

    const int64_t r0 = (int64_t)blockIdx.x * A.chunk_rows;
    const int64_t r1 = r0 + A.chunk_rows < M.rows ? r0 + A.chunk_rows : M.rows;
    for (int64_t row = r0; row < r1; ++row) {
        const int64_t mrow = (int64_t)k * M.rows + row;  // row of mu, v / cov and of the mask (k == 0 unless MASKED)
        int bad = 0;
        for (int e = tid; e < n_mc; e += 256) {
            const double x = e < L ? M.mu[mrow * L + e] : COV ? A.cov[mrow * npair + (e - L)] : M.v[mrow * L + (e - L)];
            mc[e] = x;
            if (COV) bad |= !isfinite(x);
        }
        // (a barrier: the pairs of the previous row are done with d, s, u; mc is complete)
        const int dead = __syncthreads_or(bad);
        if (dead) continue;  // uniform: the same value in every thread
        if (stager) {
            const bool live = !MASKED || ((A.mask[mrow * A.nw + (sn >> 6)] >> (sn & 63)) & 1ull);
            double eta = M.xb ? M.xb[row * N + sn] : M.b[sn];
            for (int l = 0; l < L; ++l) eta = fma(mc[l], sa[l * 64 + sc], eta);
            double arg;
            if (COV) {
                const double* C = mc + L;
                double q = 0.0;
                for (int l = 0; l < L; ++l) {
                    double t = 0.0;
                    for (int l2 = 0; l2 < L; ++l2) {
                        const int hi = max(l, l2), lo = min(l, l2);
                        t = fma(C[hi * (hi + 1) / 2 + lo], sa[l2 * 64 + sc], t);
                    }
                    if (side) uJ[l * 64 + sc] = t;
                    q = fma(sa[l * 64 + sc], t, q);
                }
                arg = fma(0.5, fmax(q, 0.0), eta);
            } else {
                arg = eta;
                for (int l = 0; l < L; ++l) {
                    const double al = sa[l * 64 + sc], vl = M.vb ? mc[L + l] : 0.0;
                    if (M.vb) arg = fma(vl, 0.5 * al * al, arg);
                    if (side) uJ[l * 64 + sc] = vl * al;
                }
            }
            const double e = sgauss ? eta : exp(clamp10(arg));
            dv[tid] = live ? M.y[row * N + sn] - e : 0.0;
            sv[tid] = live ? (sgauss ? 1.0 : e) : 0.0;
            if (side == 0) ex[sc] = live ? (sgauss ? snoise : e) : 0.0;
        }
        __syncthreads();
        double dj[4], sj[4], c[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dj[j] = dv[64 + tx + 16 * j];
            sj[j] = sv[64 + tx + 16 * j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[i][j] = 0.0;
        for (int l = 0; l < L; ++l) {
            double ai[4], uj[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ai[i] = aI[l * 64 + ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) uj[j] = uJ[l * 64 + tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) c[i][j] = fma(ai[i], uj[j], c[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double di = dv[ty + 16 * i], si = sv[ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double f = (pp >> (4 * i + j)) & 1u ? expm1(c[i][j]) : c[i][j];
                res[i][j] = fma(di, dj[j], res[i][j]);
                mod[i][j] = fma(si * sj[j], f, mod[i][j]);
            }
        }
        if (I == J && tx == ty) {  // the diagonal: the observation variance of the entry
#pragma unroll
            for (int i = 0; i < 4; ++i) mod[i][i] += ex[ty + 16 * i];
        }
    }
    double* out = A.part + ((((int64_t)k * A.tile_pairs + blockIdx.y) * A.n_chunks + blockIdx.x) * 2) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int at = (ty + 16 * i) * 64 + tx + 16 * j;
            out[at] = res[i][j];
            out[4096 + at] = mod[i][j];
        }
}

// resid, model (n_rep, N, N) = the partials of every (replica, tile pair) added in chunk order; the pairs at or below the
// diagonal are summed and their mirror images are copies.  Grid (16, tile_pairs, n_rep), 256 threads: one element each.
__global__ void __launch_bounds__(256) pair_finish(const double* part, int N, int n_chunks, int tile_pairs, double* resid,
                                                   double* model) {
    int I, J;
    pair_tiles(blockIdx.y, &I, &J);
    const int e = blockIdx.x * 256 + threadIdx.x, li = e >> 6, lj = e & 63;
    const int gi = I * 64 + li, gj = J * 64 + lj;
    if (gi >= N || gj >= N || gi < gj) return;
    const double* p = part + (((int64_t)blockIdx.z * tile_pairs + blockIdx.y) * n_chunks * 2) * 4096 + e;
    double r = 0.0, m = 0.0;
    for (int c = 0; c < n_chunks; ++c, p += 2 * 4096) {
        r += p[0];
        m += p[4096];
    }
    const int64_t base = (int64_t)blockIdx.z * N * N;
    resid[base + (int64_t)gi * N + gj] = r;
    model[base + (int64_t)gi * N + gj] = m;
    resid[base + (int64_t)gj * N + gi] = r;
    model[base + (int64_t)gj * N + gi] = m;
}

template <bool COV, bool MASKED>
int launch_pairs(vlgp_ctx* ctx, const PairArgs& A, const dim3& grid, size_t lds) {
    if (lds > 64 * 1024) CHK(vlgp_raise_lds(ctx, (const void*)pair_moments<COV, MASKED>, ctx->lds_max));
    hipLaunchKernelGGL((pair_moments<COV, MASKED>), grid, dim3(256), lds, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

}  // namespace

int launch_pair_moments(vlgp_ctx* ctx, const char* who, UnitSet& us, int vb, const double* d_mu, const double* d_cov,
                        double* d_part, double* d_resid, double* d_model) {
    const int n_rep = us.is(SET_BY_ROW) ? us.rep.n : 1;
    PairArgs A;
    A.m = fill_row_model(ctx, vlgp_rows_owner(ctx, us), us, d_cov ? 1 : vb);
    if (d_cov) A.m.mu = d_mu;
    A.cov = d_cov;
    A.mask = us.rep.d_mask;
    A.nw = us.rep.nw;
    if (A.m.rows < 1) return vlgp_fail(ctx, VLGP_ERR_STATE, "%s on an empty set", who);
    const PairLayout o = pair_layout(A.m.rows, ctx->N, n_rep, ctx->n_cu);
    if (o.tile_pairs > 65535 || n_rep > 65535)
        return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: at most 65535 channel-tile pairs and 65535 replicas per set", who);
    A.chunk_rows = (int)o.chunk_rows;
    A.n_chunks = (int)o.n_chunks;
    A.tile_pairs = (int)o.tile_pairs;
    A.part = d_part;
    const size_t lds = sizeof(double) * (size_t)pair_lds_doubles(ctx->L);
    if ((int64_t)lds > ctx->lds_max) return vlgp_fail(ctx, VLGP_ERR_ARG, "%s: %d latents need %zu bytes of LDS", who, ctx->L, lds);
    const dim3 grid((unsigned)o.n_chunks, (unsigned)o.tile_pairs, (unsigned)n_rep);
    const bool masked = us.is(SET_BY_ROW);
    CHK((d_cov ? (masked ? launch_pairs<true, true> : launch_pairs<true, false>)
               : (masked ? launch_pairs<false, true> : launch_pairs<false, false>))(ctx, A, grid, lds));
    hipLaunchKernelGGL(pair_finish, dim3(16, (unsigned)o.tile_pairs, (unsigned)n_rep), dim3(256), 0, ctx->stream, d_part, ctx->N,
                       A.n_chunks, A.tile_pairs, d_resid, d_model);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
