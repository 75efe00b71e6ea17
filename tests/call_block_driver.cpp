// Stand-alone driver of the block layouts in csrc/call_block.h (tests/test_call_block.py compiles it with the address and
// undefined-behaviour sanitizers and runs it as an ordinary program; no GPU, no Python).
//
//   call_block_driver loglik     SLOTS N_RATE WANT_RATE
//   call_block_driver predictive SLOTS N_RATE N_BLK WANT_RATE WANT_LPD
//   call_block_driver elbo       ROWS N TASKS N_BLK WANT_ROWS
//   call_block_driver forecast   ROWS L M G_LEN N_OUT
//   call_block_driver marginal   ROWS L R M N_TILES
//   call_block_driver joint      WORK ROWS L R M N_TILES K
//
// prints one line "REGION OFFSET" per region of the call's device block, in the order of the block, then "need TOTAL";
// offsets and the total count doubles.  Exit status 2 on a bad command line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "call_block.h"

static void put(const char* name, int64_t v) { printf("%s %lld\n", name, (long long)v); }
static void put_sample(const SampleLayout& s) {
    put("eps", s.eps); put("beta", s.beta); put("c", s.c); put("part", s.part); put("lw", s.lw); put("parts", s.parts);
    put("tab", s.tab);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int64_t a[8] = {};
    const int n = argc - 2;
    for (int i = 0; i < n && i < 8; ++i) a[i] = atoll(argv[i + 2]);
    const char* call = argv[1];
    if (!strcmp(call, "loglik") && n == 3) {
        const LoglikLayout o = loglik_layout(a[0], a[1], a[2] != 0);
        put("rate", o.rate); put("sums", o.sums); put("need", o.need);
    } else if (!strcmp(call, "predictive") && n == 5) {
        const PredictiveLayout o = predictive_layout(a[0], a[1], a[2], a[3] != 0, a[4] != 0);
        put("nodes", o.nodes); put("rate", o.rate); put("lpd", o.lpd); put("sums", o.sums); put("part", o.part);
        put("need", o.need);
    } else if (!strcmp(call, "elbo") && n == 5) {
        const ElboLayout o = elbo_layout(a[0], a[1], a[2], a[3], a[4] != 0);
        put("part", o.part); put("sums", o.sums); put("terms", o.terms); put("rows", o.rows); put("flag", o.flag);
        put("need", o.need);
    } else if (!strcmp(call, "forecast") && n == 5) {
        const ForecastLayout o = forecast_layout(a[0], a[1], a[2], a[3], a[4]);
        put("z", o.z); put("g", o.g); put("mu", o.mu); put("v", o.v); put("terms", o.terms); put("tab", o.tab);
        put("flag", o.flag); put("need", o.need);
    } else if (!strcmp(call, "marginal") && n == 5) {
        const MarginalLayout o = marginal_layout(a[0], a[1], a[2], a[3], a[4]);
        put("z", o.z); put_sample(o.s); put("flag", o.flag); put("need", o.need);
    } else if (!strcmp(call, "joint") && n == 7) {
        const JointLayout o = joint_layout(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
        put("work", o.work); put("stats", o.stats); put("v", o.v); put_sample(o.s); put("need", o.need);
    } else {
        return 2;
    }
    return 0;
}
