// The body of mstep_cov_accum<LT, PT> and mstep_cov_accum_masked<LT, PT> (mstep_cov.hip includes it once in each, after
// `constexpr bool MASKED`): the kernel's arguments are `MArgs A`.  Text, not a __device__ function: a body inlined into
// the kernel compiles to other code than the same statements written in it (the work-item queries are lowered before
// the inlining, without the kernel's attributes), and the unmasked kernel keeps its code.
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NA = nacc_cov<LT, PT>();
    const int N = A.N, CT = A.CT, S = A.S, L = A.L, P = A.P;
    const int TL = tri(L);
    const int tid = threadIdx.x;
    const int nl = tid % CT, s = tid / CT;
    const int n = blockIdx.y * CT + nl;
    const bool active = s < S && n < N;
    constexpr int TLT = tri(LT);
    constexpr int tile_d = MC_TILE * (LT + TLT);  // mu tile | cov tile, rows padded to the compiled size with zeros
    double* red = smem;                       // aliases the tiles after the row loop: MS_GS x (S CT)
    const int red_d = MS_GS * S * CT;
    double* etab = smem + (tile_d > red_d ? tile_d : red_d);
    fast_exp_tab_init(etab, tid);

    double al[LT], bl[PT], acc[NA];
#pragma unroll
    for (int l = 0; l < LT; ++l) al[l] = (active && l < L) ? A.a[l * N + n] : 0.0;
#pragma unroll
    for (int j = 0; j < PT; ++j) bl[j] = (active && j < P) ? A.b[j * N + n] : 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    const bool gch = (active && !MASKED) ? A.gauss[n] != 0 : false;
    if constexpr (MASKED) {
        // a channel with no observed row: every sum is 0.  One workgroup's first slice starts the diagonals of both
        // Hessians at 1: the solve finds H = (1 + eps) I, g = 0 and steps by 0, no failed factorisation at eps == 0.
        if (active && s == 0 && blockIdx.x == 0 && A.nobs[n] == 0.0) {
#pragma unroll
            for (int i = 0; i < LT; ++i) acc[LT + tri(i) + i] = 1.0;
#pragma unroll
            for (int i = 0; i < PT; ++i) acc[LT + tri(LT) + PT + tri(i) + i] = 1.0;
        }
    }

    const int64_t c0 = (int64_t)blockIdx.x * A.rows_per_wg;
    int64_t c1 = c0 + A.rows_per_wg;
    if (c1 > A.rows) c1 = A.rows;
    double* mu_t = smem;
    double* c_t = smem + MC_TILE * LT;
    // (the padding is written here, once per tile: the row loop reads LT and tri(LT) doubles a row without a predicate)
    auto copy_tile = [&](int64_t t0) {
        const int nr = (int)((c1 - t0) < MC_TILE ? (c1 - t0) : MC_TILE);
        for (int i = tid; i < nr * LT; i += blockDim.x) {
            const int r = i / LT, l = i - r * LT;
            mu_t[i] = l < L ? A.mu[(t0 + r) * L + l] : 0.0;
        }
        for (int i = tid; i < nr * TLT; i += blockDim.x) {
            const int r = i / TLT, k = i - r * TLT;
            c_t[i] = k < TL ? A.v[(t0 + r) * TL + k] : 0.0;
        }
    };
    if (c0 < c1) copy_tile(c0);
    __syncthreads();
    for (int64_t t0 = c0; t0 < c1; t0 += MC_TILE) {
        const int nr = (int)((c1 - t0) < MC_TILE ? (c1 - t0) : MC_TILE);
        const bool more = t0 + MC_TILE < c1;
        if (active && !gch) {  // Gaussian channels need no rate statistics
            for (int rr = s; rr < nr; rr += S) {
                const int64_t row = t0 + rr;
                double xv[PT];
#pragma unroll
                for (int j = 0; j < PT; ++j) xv[j] = (j < P) ? (A.x ? A.x[(row * P + j) * N + n] : 1.0) : 0.0;
                const double* cr = c_t + rr * TLT;
                double mt[LT], q[LT];
#pragma unroll
                for (int l = 0; l < LT; ++l) q[l] = 0.0;
                // q = C a over the packed lower triangle: each pair once, both of its products
#pragma unroll
                for (int i = 0; i < LT; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        const double c = cr[tri(i) + j];
                        q[i] = fma(c, al[j], q[i]);
                        if (j < i) q[j] = fma(c, al[i], q[j]);
                    }
                double eta = 0.0;
#pragma unroll
                for (int j = 0; j < PT; ++j) eta = fma(xv[j], bl[j], eta);
                double s2 = 0.0;
#pragma unroll
                for (int l = 0; l < LT; ++l) {
                    const double m = mu_t[rr * LT + l];
                    eta = fma(m, al[l], eta);
                    s2 = fma(al[l], q[l], s2);
                    mt[l] = m + q[l];
                }
                double rate = trunc_exp_tab64(fma(0.5, s2, eta), etab);
                if constexpr (MASKED) {
                    // is y[row, n] observed?  The lane's 32-bit half of the row's mask word, asked where the answer is used
                    const int nw = (N + 63) >> 6;
                    const unsigned half = reinterpret_cast<const unsigned*>(A.mask)[row * (2 * nw) + (n >> 5)];
                    rate = ((half >> (n & 31)) & 1u) == 0u ? rate : 0.0;
                }
                // the Hessian reads the row's C from LDS again: held in registers across the exponential, its tri(L)
                // doubles spill at five latents and 128 registers
                asm volatile("" ::: "memory");
                int k = 0;
#pragma unroll
                for (int l = 0; l < LT; ++l) { acc[k] = fma(rate, mt[l], acc[k]); ++k; }
#pragma unroll
                for (int i = 0; i < LT; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        const double c = cr[tri(i) + j];
                        acc[k] = fma(rate, fma(mt[i], mt[j], c), acc[k]);
                        ++k;
                    }
#pragma unroll
                for (int j = 0; j < PT; ++j) { acc[k] = fma(xv[j], rate, acc[k]); ++k; }
#pragma unroll
                for (int i = 0; i < PT; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) { acc[k] = fma(xv[i] * xv[j], rate, acc[k]); ++k; }
            }
        }
        if (more) {
            __syncthreads();  // everybody is done with the tile
            copy_tile(t0 + MC_TILE);
        }
        __syncthreads();
    }
    // slices -> one partial per workgroup, as mstep_accum
    const int K = 2 * L + TL + P + tri(P);
    const int SC = S * CT;
#pragma unroll
    for (int g0 = 0; g0 < NA; g0 += MS_GS) {
        if (s < S) {
#pragma unroll
            for (int j = 0; j < MS_GS; ++j)
                if (g0 + j < NA) red[j * SC + s * CT + nl] = active ? acc[g0 + j] : 0.0;
        }
        __syncthreads();
        for (int o = tid; o < MS_GS * CT; o += blockDim.x) {
            const int j = o / CT, c = o - j * CT;
            int ke = -1;
#pragma unroll
            for (int jj = 0; jj < MS_GS; ++jj)
                if (g0 + jj < NA && jj == j) ke = mcov_slot<LT, PT>(g0 + jj, L, P);
            const int nn = blockIdx.y * CT + c;
            if (ke >= 0 && nn < N) {
                double t = 0.0;
                for (int qs = 0; qs < S; ++qs) t += red[j * SC + qs * CT + c];
                A.partial[((int64_t)blockIdx.x * K + ke) * N + nn] = t;
            }
        }
        if (g0 + MS_GS < NA) __syncthreads();
    }
    for (int o = tid; o < L * CT; o += blockDim.x) {  // the r'v slots: zeros
        const int l = o / CT, nn = blockIdx.y * CT + (o - l * CT);
        if (nn < N) A.partial[((int64_t)blockIdx.x * K + L + TL + l) * N + nn] = 0.0;
    }
