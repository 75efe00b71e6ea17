// Host driver of tests/test_calibration_host.py: prints the regions of vlgp_calibration's device block
// (csrc/call_block.h, calibration_layout) as "<region> <offset in doubles>" lines, then "groups" and "need".
//   calibration_layout_driver slots n_rate n_blk n_bins n_levels want_cdf
#include <cstdio>
#include <cstdlib>

#include "call_block.h"

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s slots n_rate n_blk n_bins n_levels want_cdf\n", argv[0]);
        return 2;
    }
    long long a[6];
    for (int i = 0; i < 6; ++i) a[i] = std::atoll(argv[i + 1]);
    const CalibrationLayout o = calibration_layout(a[0], a[1], a[2], a[3], a[4], a[5] != 0);
    std::printf("nodes %lld\nlevels %lld\ncdf %lld\nsums %lld\npart %lld\ngroups %lld\nneed %lld\n", (long long)o.nodes,
                (long long)o.levels, (long long)o.cdf, (long long)o.sums, (long long)o.part, (long long)o.groups,
                (long long)o.need);
    return 0;
}
