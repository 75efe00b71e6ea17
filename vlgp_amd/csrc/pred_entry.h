// What the kernels of the predictive distribution share (predictive.hip, calibrate.hip): the node tables of the
// Gauss-Hermite rule in LDS and the Poisson-lognormal integral by the mode-centred rule.  Device helpers only; no kernels.
#pragma once
#include "row_walk.h"

#define PRED_NODES 64  // most nodes of a rule (the host checks)

struct Nodes {
    int n;
    const double* tab;  // global: z (n) | lwa (n)
};

// the tables in LDS; the caller synchronises
struct NodeTables { double z[PRED_NODES], lwa[PRED_NODES]; };
__device__ __forceinline__ void nodes_stage(const Nodes& Q, NodeTables& t) {
    if ((int)threadIdx.x < Q.n) {
        t.z[threadIdx.x] = Q.tab[threadIdx.x];
        t.lwa[threadIdx.x] = Q.tab[Q.n + threadIdx.x];
    }
}

// log int Poisson(y | exp(min(eta, 10))) N(eta; m, s2) d eta + lgamma(y + 1), s2 >= 1e-30
__device__ __forceinline__ double poisson_lognormal(double yv, double m, double s2, int nq, const double* zt,
                                                    const double* lt) {
    const double is2 = 1.0 / s2;
    double e = m;
    if (yv > exp(clamp10(m))) e = fmin(log(yv), m + yv * s2);
#pragma unroll 1
    for (int it = 0; it < 8; ++it) {
        const double x = exp(clamp10(e));
        e -= (yv - x - (e - m) * is2) / (-x - is2);
    }
    const double h = s2 * exp(clamp10(e)) + 1.0;
    const double tau = sqrt(s2) / sqrt(h);
    const double hs = 0.5 * is2;
    double top = -INFINITY, acc = 0.0;
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {
        const double eta = fma(tau, zt[q], e);
        const double c = clamp10(eta), d = eta - m;
        const double t = lt[q] + yv * c - exp(c) - d * d * hs;
        if (t > top) {  // (exp(-inf) = 0 at the first node; a NaN never enters here and poisons acc below)
            acc = acc * exp(top - t) + 1.0;
            top = t;
        } else {
            acc += exp(t - top);
        }
    }
    return -0.5 * log(h) + (top + log(acc));
}
