// M-step under a full Gaussian posterior per row (vlgp_mstep_cov).  Part of mstep.hip's translation unit
// (included at its end): it launches that file's PREP, noise, reduce and solve kernels unchanged and adds the one pass
// that differs, the rate-dependent sums of a Newton iteration.
//
// core.mstep (vlgp/core.py:129-249) with the diagonal v of a row replaced by the row's L x L covariance C_t.  With
// q_tn = C_t a_n and s2_tn = a_n . q_tn the rate is r = exp(eta + s2 / 2) and, per Poisson channel n,
//     grad_a = mu' y_n - sum_t r_tn (mu_t + q_tn)
//     nhess_a = sum_t r_tn [(mu_t + q_tn)(mu_t + q_tn)' + C_t]
// while grad_b, nhess_b, the jitter, the clips and the learning-rate fall-back are mstep.hip's.  A Gaussian channel's
// least squares take M = mu'mu + sum_t C_t.  The y-dependent halves, the moments of mu and the noise read mu, y, x
// only: the existing kernels on the uploaded mu.
//
// Partial sums in K_NEWTON's layout, (mu + q)'r | Hessian | r'v | x'r | x' diag(r) x, the r'v slots written as zeros
// (sum_t r C_t is folded into the Hessian): sum_partials_kernel, mstep_sum_solve_kernel and mstep_solve_kernel follow
// unchanged.  Fixed-order sums, no atomics on doubles.

// rows of (mu | cov) staged in LDS per step: L + L (L + 1) / 2 doubles a row, 49 920 bytes at ten latents -- under the
// 64 KB a kernel gets without a raised ceiling.  (This M-step runs alone on the device: no H-step round beside it.)
#ifndef MC_TILE
#define MC_TILE 96
#endif

template <int LT, int PT>
__host__ __device__ constexpr int nacc_cov() { return LT + tri(LT) + PT + tri(PT); }

// Where accumulator k of the padded (LT, PT) layout sits in K_NEWTON's exact (L, P) layout, the L slots of r'v skipped; -1
// for padding.  (A packed pair keeps its place whatever L is; k is a constant wherever this is called: no table of slots
// lives in registers beside the accumulators.)
template <int LT, int PT>
__device__ __forceinline__ int mcov_slot(int k, int L, int P) {
    if (k < LT) return k < L ? k : -1;
    k -= LT;
    if (k < tri(LT)) {
        int i = 0;
        while (tri(i + 1) <= k) ++i;
        return i < L ? L + k : -1;
    }
    k -= tri(LT);
    if (k < PT) return k < P ? 2 * L + tri(L) + k : -1;
    k -= PT;
    int i = 0;
    while (tri(i + 1) <= k) ++i;
    return i < P ? 2 * L + tri(L) + P + k : -1;
}

// lane <-> channel, S row slices per workgroup, as mstep_accum; A.v is cov (rows, tri(L)), pair (l, l'), l' <= l, at
// l (l + 1) / 2 + l' whatever L is: in a row padded to tri(LT) every pair keeps its place.
//
// MASKED (vlgp_mstep_cov_masked): a masked fit set, every channel over its observed rows.  The sums are
// linear in the rate, so a missing entry puts 0 there by a select, as mstep_accum<..., K_NEWTON | K_MASKED, ...> does --
// never a product with 0 -- and with no bit set the sums are the unmasked kernel's, bit for bit.  A.mask sits in the
// slot of A.gauss (a masked handle has no Gaussian channel), A.nobs in the slot of A.mean.  One body
// (mstep_cov_accum.inc) behind two kernel names: the unmasked kernel keeps its symbol and its code.
template <int LT, int PT>
__global__ void __launch_bounds__(512, (LT <= 5 ? 4 : (LT <= 8 ? 2 : 1))) mstep_cov_accum(MArgs A) {
    constexpr bool MASKED = false;
#include "mstep_cov_accum.inc"
}
template <int LT, int PT>
__global__ void __launch_bounds__(512, (LT <= 5 ? 4 : (LT <= 8 ? 2 : 1))) mstep_cov_accum_masked(MArgs A) {
    constexpr bool MASKED = true;
#include "mstep_cov_accum.inc"
}

// first row of (mu | cov) that holds a non-finite value: *first = its index, left alone (rows) when all are finite.
// An integer minimum: the answer does not depend on the order of the updates.
__global__ void __launch_bounds__(256)
mcov_first_bad_row(int64_t rows, int L, const double* mu, const double* cov, unsigned long long* first) {
    const int TL = tri(L);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < rows; t += (int64_t)gridDim.x * 256) {
        bool bad = false;
        for (int l = 0; l < L; ++l) bad = bad || !(fabs(mu[t * L + l]) < INFINITY);
        for (int k = 0; k < TL; ++k) bad = bad || !(fabs(cov[t * TL + k]) < INFINITY);
        if (bad) atomicMin(first, (unsigned long long)t);
    }
}

// partial[g][k] = sum of cov[t][k] over workgroup g's rows: grid (G, tri(L)), thread i of workgroup g adds the rows
// t = 256 g + i, 256 g + i + 256 G, ... (latent_moments_kernel's striding), then that kernel's tree over the 256 threads
__global__ void __launch_bounds__(256) mcov_sum_kernel(int TL, int64_t rows, const double* cov, double* partial) {
    __shared__ double red[256];
    const int k = blockIdx.y;
    double acc = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < rows; t += (int64_t)gridDim.x * 256) acc += cov[t * TL + k];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * TL + k] = red[0];
}
// the moments the Gaussian channels' solve reads (SolveArgs::lat): gram of mu + sum_t C_t | sum mu | zeros in place of
// sum v | the rest as it is
__global__ void mcov_lat_kernel(int L, const double* lat, const double* csum, double* out) {
    const int TL = tri(L), K = TL + 3 * L + 1;
    for (int i = threadIdx.x; i < K; i += blockDim.x)
        out[i] = i < TL ? lat[i] + csum[i] : (i >= TL + L && i < TL + 2 * L) ? 0.0 : lat[i];
}

static size_t mcov_lds(const Geometry& g, int LT) {
    const size_t tile = (size_t)MC_TILE * (LT + tri(LT)), redb = (size_t)MS_GS * g.S * g.CT;
    return ((tile > redb ? tile : redb) + 64) * 8;
}
template <int LT>
static int launch_cov_accum_p(vlgp_ctx* ctx, const Geometry& g, const MArgs& A) {
    const dim3 grid(g.G, g.tiles), blk(g.nthr);
    const size_t lds = mcov_lds(g, LT);
    hipStream_t st = ctx->mstream;
    switch (accum_pt(A.P)) {
        case 1: hipLaunchKernelGGL((mstep_cov_accum<LT, 1>), grid, blk, lds, st, A); break;
        case 2: hipLaunchKernelGGL((mstep_cov_accum<LT, 2>), grid, blk, lds, st, A); break;
        case 4: hipLaunchKernelGGL((mstep_cov_accum<LT, 4>), grid, blk, lds, st, A); break;
        case 8: hipLaunchKernelGGL((mstep_cov_accum<LT, 8>), grid, blk, lds, st, A); break;
        default: return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_mstep_cov: more than 8 regressors (P = %d)", A.P);
    }
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
static int launch_cov_accum(vlgp_ctx* ctx, const Geometry& g, const MArgs& A) {
    switch (A.L <= 10 ? accum_lt(A.L) : 0) {
        case 2: return launch_cov_accum_p<2>(ctx, g, A);
        case 3: return launch_cov_accum_p<3>(ctx, g, A);
        case 5: return launch_cov_accum_p<5>(ctx, g, A);
        case 8: return launch_cov_accum_p<8>(ctx, g, A);
        case 10: return launch_cov_accum_p<10>(ctx, g, A);
    }
    return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_mstep_cov: more than 10 latents (L = %d)", A.L);
}
// the same matrix of the masked kernel (A.mask, A.nobs set): the unmasked launch's grid, workgroup and LDS
template <int LT>
static int launch_cov_masked_p(vlgp_ctx* ctx, const Geometry& g, const MArgs& A) {
    const dim3 grid(g.G, g.tiles), blk(g.nthr);
    const size_t lds = mcov_lds(g, LT);
    hipStream_t st = ctx->mstream;
    switch (accum_pt(A.P)) {
        case 1: hipLaunchKernelGGL((mstep_cov_accum_masked<LT, 1>), grid, blk, lds, st, A); break;
        case 2: hipLaunchKernelGGL((mstep_cov_accum_masked<LT, 2>), grid, blk, lds, st, A); break;
        case 4: hipLaunchKernelGGL((mstep_cov_accum_masked<LT, 4>), grid, blk, lds, st, A); break;
        case 8: hipLaunchKernelGGL((mstep_cov_accum_masked<LT, 8>), grid, blk, lds, st, A); break;
        default: return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_mstep_cov_masked: more than 8 regressors (P = %d)", A.P);
    }
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}
static int launch_cov_masked(vlgp_ctx* ctx, const Geometry& g, const MArgs& A) {
    switch (A.L <= 10 ? accum_lt(A.L) : 0) {
        case 2: return launch_cov_masked_p<2>(ctx, g, A);
        case 3: return launch_cov_masked_p<3>(ctx, g, A);
        case 5: return launch_cov_masked_p<5>(ctx, g, A);
        case 8: return launch_cov_masked_p<8>(ctx, g, A);
        case 10: return launch_cov_masked_p<10>(ctx, g, A);
    }
    return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_mstep_cov_masked: more than 10 latents (L = %d)", A.L);
}

int launch_mcov_first_bad_row(vlgp_ctx* ctx, int64_t rows, const double* d_mu, const double* d_cov, unsigned long long* d_first,
                              hipStream_t st) {
    int64_t G = (rows + 255) / 256;
    if (G > 1024) G = 1024;
    if (G < 1) G = 1;
    hipLaunchKernelGGL(mcov_first_bad_row, dim3((unsigned)G), dim3(256), 0, st, rows, ctx->L, d_mu, d_cov, d_first);
    HIPCHK(ctx, hipGetLastError());
    return VLGP_OK;
}

// One rank, the compiled sizes (L <= 10, P <= 8), a set that is not replicated: the caller has checked.  Everything on
// ctx->mstream with the M-step lane's workspace, launch by launch (no captured graph: the moments' block is the call's).
// A masked fit set (vlgp_mstep_cov_masked; no Gaussian channel on the handle: checked as well) takes what the masked
// launch_mstep takes -- K_PREP | K_MASKED, the noise by the two masked passes over each channel's own observed rows --
// with mstep_cov_accum_masked as the Newton pass.
int launch_mstep_cov(vlgp_ctx* ctx, UnitSet& us, const double* d_mu, const double* d_cov, int n_iter, int use_hessian,
                     double eps, double lr, double da_bound, double db_bound) {
    const int N = ctx->N, L = ctx->L, P = ctx->P;
    const bool masked = us.is(SET_MASKED_FIT);
    if (masked && (!us.rep.d_mask || !us.rep.d_nobs)) return vlgp_fail(ctx, VLGP_ERR_STATE, "vlgp_mstep_cov_masked: the set has no mask");
    const int km = masked ? K_MASKED : 0;
    const Geometry g = plan(ctx, us.rows);
    const int Kp = nstat_rt(L, P, K_PREP), Kn = nstat_rt(L, P, K_NEWTON);
    const int Kl = tri(L) + 3 * L + 1;
    const int Kmax = Kp > Kn ? Kp : Kn;
    // workspace: prep | stats | lat | lat of the Gaussian solve | sum of cov | noise1 | mean | ticket | partial
    const int64_t o_prep = 0, o_stats = o_prep + (int64_t)Kp * N, o_lat = o_stats + (int64_t)Kn * N, o_latg = o_lat + Kl + 8;
    const int64_t o_csum = o_latg + Kl + 8, o_s1 = o_csum + tri(L) + 8, o_mean = o_s1 + N, o_tick = o_mean + N, o_part = o_tick + 2;
    int64_t part_len = (int64_t)g.G * Kmax * N;
    if (part_len < 256LL * Kl) part_len = 256LL * Kl;
    CHK(vlgp_ensure_work_m(ctx, o_part + part_len));
    double* W = ctx->d_work_m;
    hipStream_t st = ctx->mstream;
    double *d_prep = W + o_prep, *d_stats = W + o_stats, *d_lat = W + o_lat, *d_latg = W + o_latg, *d_csum = W + o_csum,
           *d_s1 = W + o_s1, *d_mean = W + o_mean, *d_part = W + o_part;
    unsigned* d_ticket = reinterpret_cast<unsigned*>(W + o_tick);
    HIPCHK(ctx, hipMemsetAsync(d_ticket, 0, sizeof(double) * 2, st));

    MArgs A;
    A.N = N; A.L = L; A.P = P; A.rows = us.rows; A.rows_per_wg = g.rows_per_wg; A.CT = g.CT; A.S = g.S;
    A.y = us.y; A.x = us.x_ones ? nullptr : us.x; A.mu = d_mu;
    A.v = d_cov;  // (the PREP and noise passes stage rows x L doubles of it beside mu and read none of them)
    A.a = ctx->d_a; A.b = ctx->d_b; A.gauss = ctx->d_gauss; A.mean = d_mean; A.partial = d_part;
    if (masked) A.mask = us.rep.d_mask;  // (in the slot of gauss: the Newton launch gets nobs in the slot of mean)
    auto reduce_to = [&](int K, double* dst) -> int {
        const int64_t n = (int64_t)K * N;
        hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((n + 63) / 64)), dim3(512), 0, st, d_part, g.G, n, dst);
        HIPCHK(ctx, hipGetLastError());
        return VLGP_OK;
    };

    // sweep-invariant moments: mu'y, x'y, x'mu, x'x; gram and column sums of mu; sum_t C_t for the Gaussian channels
    CHK(launch_accum(ctx, K_PREP | km, g, A));
    CHK(reduce_to(Kp, d_prep));
    {
        int G = (int)((us.rows + 255) / 256);
        if (G > 256) G = 256;
        if (G < 1) G = 1;
        switch (accum_lt(L)) {
            case 2: launch_lat_t<2>(st, G, L, us.rows, d_mu, nullptr, nullptr, d_part); break;
            case 3: launch_lat_t<3>(st, G, L, us.rows, d_mu, nullptr, nullptr, d_part); break;
            case 5: launch_lat_t<5>(st, G, L, us.rows, d_mu, nullptr, nullptr, d_part); break;
            case 8: launch_lat_t<8>(st, G, L, us.rows, d_mu, nullptr, nullptr, d_part); break;
            default: launch_lat_t<10>(st, G, L, us.rows, d_mu, nullptr, nullptr, d_part); break;
        }
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(sum_partials_kernel, dim3((Kl + 63) / 64), dim3(512), 0, st, d_part, G, (int64_t)Kl, d_lat);
        if (ctx->n_gauss > 0) {
            hipLaunchKernelGGL(mcov_sum_kernel, dim3(G, tri(L)), dim3(256), 0, st, tri(L), us.rows, d_cov, d_part);
            hipLaunchKernelGGL(sum_partials_kernel, dim3((tri(L) + 63) / 64), dim3(512), 0, st, d_part, G, (int64_t)tri(L), d_csum);
            hipLaunchKernelGGL(mcov_lat_kernel, dim3(1), dim3(128), 0, st, L, d_lat, d_csum, d_latg);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    const double total_rows = (double)us.rows;

    SolveArgs S;
    S.N = N; S.L = L; S.P = P; S.use_hessian = use_hessian; S.eps = eps; S.lr = lr;
    S.da_bound = da_bound; S.db_bound = db_bound;
    S.prep = d_prep; S.stats = d_stats; S.lat = ctx->n_gauss > 0 ? d_latg : d_lat; S.gauss = ctx->d_gauss;
    S.a = ctx->d_a; S.b = ctx->d_b; S.da = ctx->d_da; S.db = ctx->d_db; S.fail = ctx->d_fail_m;
    S.hws = nullptr;

    const bool any_poisson = ctx->n_gauss < N;
    for (int it = 0; it < n_iter; ++it) {
        if (it == n_iter - 1) {
            // noise = var(y - eta) with the parameters entering the last iteration (core.py:177), as launch_mstep
            if (!masked && !noise_by_passes(ctx)) {
                hipLaunchKernelGGL(noise_stats_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, L, P, total_rows, d_prep, d_lat,
                                   ctx->d_a, ctx->d_b, ctx->d_noise);
                HIPCHK(ctx, hipGetLastError());
            } else {
                CHK(launch_accum(ctx, K_NOISE1 | km, g, A));
                CHK(reduce_to(1, d_s1));
                if (masked) hipLaunchKernelGGL(noise_mean_nobs_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, us.rep.d_nobs, d_s1, d_mean);
                else hipLaunchKernelGGL(noise_mean_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, total_rows, d_s1, d_mean);
                CHK(launch_accum(ctx, K_NOISE2 | km, g, A));
                CHK(reduce_to(1, d_s1));
                if (masked) hipLaunchKernelGGL(noise_final_nobs_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, us.rep.d_nobs, d_s1, ctx->d_noise);
                else hipLaunchKernelGGL(noise_final_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, total_rows, d_s1, ctx->d_noise);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        if (any_poisson) {
            if (masked) {
                MArgs An = A;
                An.nobs = us.rep.d_nobs;  // (the Newton launch reads no mean)
                CHK(launch_cov_masked(ctx, g, An));
            } else {
                CHK(launch_cov_accum(ctx, g, A));
            }
            launch_sum_solve(ctx, st, d_part, g.G, (int64_t)Kn * N, d_stats, d_ticket, S);
            HIPCHK(ctx, hipGetLastError());
            continue;
        }
        hipLaunchKernelGGL(mstep_solve_kernel, dim3((N + 63) / 64), dim3(64), 0, st, S);
        HIPCHK(ctx, hipGetLastError());
    }
    return VLGP_OK;
}
