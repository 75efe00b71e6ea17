// Host driver of tests/test_lag_host.py: prints the regions of vlgp_lag_moments' device block and the launch sizes
// (csrc/call_block.h, lag_layout) as "<name> <value>" lines, the LDS of the two wave kernels, and what lag_refusal says
// to the call (its status and, behind it, the number its message names).
//   lag_layout_driver rows N L n_rep tasks K vb n_cu rp world
#include <cstdio>
#include <cstdlib>

#include "call_block.h"

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s rows N L n_rep tasks K vb n_cu rp world\n", argv[0]);
        return 2;
    }
    long long a[10];
    for (int i = 0; i < 10; ++i) a[i] = std::atoll(argv[i + 1]);
    // as the call does: the arguments first (a lag out of range sizes nothing), then the layout, then the workspace
    const LagRefusal first = lag_refusal((int)a[9], (int)a[5], 0, 0);
    if (first.status) {
        char text[512];
        std::snprintf(text, sizeof text, first.text, first.arg);
        std::fprintf(stderr, "%s\n", text);
        std::printf("refusal %d\nrefusal_arg %lld\n", first.status, first.arg);
        return 0;
    }
    const LagLayout o = lag_layout(a[0], a[1], a[2], a[3], a[4], a[5], a[6] != 0, a[7]);
    std::printf("w %lld\nc %lld\nflag %lld\npart %lld\nresid %lld\nmodel %lld\ncount %lld\ntiles %lld\nchunk_rows %lld\n"
                "n_chunks %lld\nc_doubles %lld\nneed %lld\n",
                (long long)o.w, (long long)o.c, (long long)o.flag, (long long)o.part, (long long)o.resid, (long long)o.model,
                (long long)o.count, (long long)o.tiles, (long long)o.chunk_rows, (long long)o.n_chunks, (long long)o.c_doubles,
                (long long)o.need);
    const long long rs = a[8] | 1;
    std::printf("task_lds_doubles %lld\nmoments_lds_bytes %lld\nmin_chunk %d\nlag_group %d\nlag_max %d\n",
                (long long)lag_task_lds_doubles(a[8], rs, a[5]), (long long)lag_moments_lds_bytes(a[2], a[5]), LAG_MIN_CHUNK,
                LAG_GROUP, LAG_MAX);
    const LagRefusal no = lag_refusal((int)a[9], (int)a[5], (int)a[8], o.c_doubles);
    std::printf("refusal %d\nrefusal_arg %lld\n", no.status, no.status ? no.arg : 0LL);
    if (no.status) {
        char text[512];
        std::snprintf(text, sizeof text, no.text, no.arg);
        std::fprintf(stderr, "%s\n", text);
    }
    return 0;
}
