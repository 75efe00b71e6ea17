// CPU build of vlgp_amd/csrc/fast_exp.h for the tests (g++ -O2 -mfma -ffp-contract=off -Ihip_shim): the header is
// included UNCHANGED behind tests/native/hip_shim/hip/hip_runtime.h; the five rate exponentials and the two tables are
// exposed with C linkage.  The kinds are the probe kinds of vlgp_debug_npx (include/vlgp_hip.h).  Test infrastructure only.
#include "../../vlgp_amd/csrc/fast_exp.h"

namespace {
double g_tab64[64], g_tab256[256];
bool g_ready = false;
// the tables as a workgroup fills them in LDS: every thread of one workgroup calls the product's init
void fill_tables() {
    if (g_ready) return;
    for (int tid = 0; tid < (int)blockDim.x; ++tid) {
        fast_exp_tab_init(g_tab64, tid);
        fast_exp_tab256_init(g_tab256, tid);
    }
    g_ready = true;
}
}  // namespace

extern "C" {
// 4: fast_exp(clamp10(x))  5: fast_exp_tab<false>(clamp10(x))  6: trunc_exp_tab64(x)
// 7: fast_exp_tab256<false>(clamp10(x))  8: trunc_exp_tab256(x); returns 0, or -1 for another kind
int fx_eval(int kind, const double* x, double* y, long n) {
    fill_tables();
    if (kind < 4 || kind > 8) return -1;
    for (long i = 0; i < n; ++i) {
        const double v = x[i];
        if (kind == 4) y[i] = fast_exp(clamp10(v));
        else if (kind == 5) y[i] = fast_exp_tab<false>(clamp10(v), g_tab64);
        else if (kind == 6) y[i] = trunc_exp_tab64(v, g_tab64);
        else if (kind == 7) y[i] = fast_exp_tab256<false>(clamp10(v), g_tab256);
        else y[i] = trunc_exp_tab256(v, g_tab256);
    }
    return 0;
}
// the constant tables themselves and what the init functions copied
void fx_tables(double* t64, double* t256, double* lds64, double* lds256) {
    fill_tables();
    for (int j = 0; j < 64; ++j) { t64[j] = vlgp_exp2_tab64[j]; lds64[j] = g_tab64[j]; }
    for (int j = 0; j < 256; ++j) { t256[j] = vlgp_exp2_tab256[j]; lds256[j] = g_tab256[j]; }
}
}
