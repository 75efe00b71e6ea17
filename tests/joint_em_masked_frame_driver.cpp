// Host driver of tests/test_joint_em_masked_host.py: the host frame of vlgp_mstep_cov_masked as csrc/call_block.h states it.
//   joint_em_masked_frame_driver layout rows L                                   -> "first", "mu", "cov", "need" <offset in doubles>
//   joint_em_masked_frame_driver refuse n_gauss L P generic world mu cov n_iter  -> "status <int>" and "text <message>" (mu, cov: 0 = null)
//   joint_em_masked_frame_driver walk rows L                                     -> fills a host block of `need` doubles region by
//                                                                                   region and reads every region back: "ok <need>"
// The block is mstep_cov_layout's, the one vlgp_mstep_cov uses: the masked call adds no region (the mask and the counts of
// observed rows belong to the set).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "call_block.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 2; i < argc && i < 10; ++i) a[i - 2] = std::atoll(argv[i]);
    if (!std::strcmp(argv[1], "layout") && argc == 4) {
        const MstepCovLayout o = mstep_cov_layout(a[0], a[1]);
        std::printf("first %lld\nmu %lld\ncov %lld\nneed %lld\n", (long long)o.first, (long long)o.mu, (long long)o.cov,
                    (long long)o.need);
        return 0;
    }
    if (!std::strcmp(argv[1], "refuse") && argc == 10) {
        static const double moments[1] = {0.0};
        const MstepCovRefusal r = mstep_cov_masked_refusal((int)a[0], (int)a[1], (int)a[2], a[3] != 0, (int)a[4],
                                                           a[5] ? moments : nullptr, a[6] ? moments : nullptr, (int)a[7]);
        std::printf("status %d\ntext %s\n", r.status, r.text ? r.text : "");
        return 0;
    }
    if (!std::strcmp(argv[1], "walk") && argc == 4) {
        const long long rows = a[0], L = a[1], TL = L * (L + 1) / 2;
        const MstepCovLayout o = mstep_cov_layout(rows, L);
        std::vector<double> block((size_t)o.need, -1.0);  // exactly `need` doubles: a region past it is the sanitizer's find
        long long first = rows;
        std::memcpy(block.data() + o.first, &first, sizeof(first));
        for (long long i = 0; i < rows * L; ++i) block[(size_t)(o.mu + i)] = 1.0;
        for (long long i = 0; i < rows * TL; ++i) block[(size_t)(o.cov + i)] = 2.0;
        long long back = -1;
        std::memcpy(&back, block.data() + o.first, sizeof(back));
        if (back != rows) return 1;  // (the regions do not overlap: every value is the one its region wrote)
        for (long long i = 0; i < rows * L; ++i)
            if (block[(size_t)(o.mu + i)] != 1.0) return 1;
        for (long long i = 0; i < rows * TL; ++i)
            if (block[(size_t)(o.cov + i)] != 2.0) return 1;
        for (long long i = 0; i < o.need; ++i)
            if (block[(size_t)i] == -1.0) return 1;  // ... and together they cover the block
        std::printf("ok %lld\n", (long long)o.need);
        return 0;
    }
    return 2;
}
