// Host driver of tests/test_pair_host.py: prints the regions of vlgp_pair_moments' device block and the launch sizes
// (csrc/call_block.h, pair_layout) as "<name> <value>" lines, then the sibling's mu, cov behind it (moments_layout over
// post_rows rows) and the LDS doubles of a workgroup.
//   pair_layout_driver rows N n_rep n_cu post_rows L
#include <cstdio>
#include <cstdlib>

#include "call_block.h"

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s rows N n_rep n_cu post_rows L\n", argv[0]);
        return 2;
    }
    long long a[6];
    for (int i = 0; i < 6; ++i) a[i] = std::atoll(argv[i + 1]);
    const PairLayout o = pair_layout(a[0], a[1], a[2], a[3]);
    const MomentsLayout m = moments_layout(o.need, a[4], a[5]);
    std::printf("part %lld\nresid %lld\nmodel %lld\ntiles %lld\ntile_pairs %lld\nchunk_rows %lld\nn_chunks %lld\nneed %lld\n",
                (long long)o.part, (long long)o.resid, (long long)o.model, (long long)o.tiles, (long long)o.tile_pairs,
                (long long)o.chunk_rows, (long long)o.n_chunks, (long long)o.need);
    std::printf("mu %lld\ncov %lld\nmoments_need %lld\nlds_doubles %lld\nmin_chunk %d\n", (long long)m.mu, (long long)m.cov,
                (long long)m.need, (long long)pair_lds_doubles(a[5]), PAIR_MIN_CHUNK);
    return 0;
}
