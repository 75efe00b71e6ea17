// Host driver of tests/test_joint_cov_host.py: prints the regions of the device blocks that vlgp_joint_posterior and the
// _cov row scores add to csrc/call_block.h as "<region> <offset in doubles>" lines.
//   joint_cov_layout_driver moments sibling_need post_rows L      -> mu, cov, need
//   joint_cov_layout_driver posterior work rows L M               -> work, stats, cov, need
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "call_block.h"

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) {
        std::fprintf(stderr, "usage: %s moments sibling_need post_rows L | posterior work rows L M\n", argv[0]);
        return 2;
    }
    long long a[4] = {0, 0, 0, 0};
    for (int i = 2; i < argc; ++i) a[i - 2] = std::atoll(argv[i]);
    if (!std::strcmp(argv[1], "moments") && argc == 5) {
        const MomentsLayout o = moments_layout(a[0], a[1], a[2]);
        std::printf("mu %lld\ncov %lld\nneed %lld\n", (long long)o.mu, (long long)o.cov, (long long)o.need);
        return 0;
    }
    if (!std::strcmp(argv[1], "posterior") && argc == 6) {
        const JointPosteriorLayout o = joint_posterior_layout(a[0], a[1], a[2], a[3]);
        std::printf("work %lld\nstats %lld\ncov %lld\nneed %lld\n", (long long)o.work, (long long)o.stats, (long long)o.cov,
                    (long long)o.need);
        return 0;
    }
    return 2;
}
