// Host driver of tests/test_joint_hstep_host.py: what vlgp_joint_posterior_moments adds to csrc/call_block.h, printed as
// "<name> <value>" lines.
//   joint_hstep_layout_driver layout work rows L M window   -> the regions of the call's device block, in doubles
//   joint_hstep_layout_driver refusal window rp n_windows   -> status and, when refused, the formatted text
//   joint_hstep_layout_driver windows T window              -> n, the number of windows of a unit of T rows
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "call_block.h"

int main(int argc, char** argv) {
    long long a[5] = {0, 0, 0, 0, 0};
    for (int i = 2; i < argc && i < 7; ++i) a[i - 2] = std::atoll(argv[i]);
    if (argc == 7 && !std::strcmp(argv[1], "layout")) {
        const JointMomentsLayout o = joint_moments_layout(a[0], a[1], a[2], a[3], a[4]);
        std::printf("work %lld\nstats %lld\ncov %lld\nposterior_need %lld\npart %lld\nS %lld\nneed %lld\n", (long long)o.p.work,
                    (long long)o.p.stats, (long long)o.p.cov, (long long)o.p.need, (long long)o.part, (long long)o.S,
                    (long long)o.need);
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "refusal")) {
        const JointMomentsRefusal r = joint_moments_refusal((int)a[0], (int)a[1], a[2]);
        std::printf("status %d\n", r.status);
        if (r.status) {
            char text[256];
            std::snprintf(text, sizeof text, r.text, r.arg);
            std::printf("text %s\n", text);
        }
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "windows")) {
        std::printf("n %lld\n", (long long)joint_unit_windows(a[0], a[1]));
        return 0;
    }
    std::fprintf(stderr, "usage: %s layout work rows L M window | refusal window rp n_windows | windows T window\n", argv[0]);
    return 2;
}
