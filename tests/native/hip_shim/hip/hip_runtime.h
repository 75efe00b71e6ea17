// Stand-in for <hip/hip_runtime.h> so that g++ can compile vlgp_amd/csrc/fast_exp.h UNCHANGED for the CPU
// (tests/native/fast_exp_harness.cpp).  Only what that header uses.  Test infrastructure only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))

// the workgroup size fast_exp_tab256_init strides by (the harness "launches" one workgroup, thread by thread)
struct shim_dim3 {
    unsigned x, y, z;
};
static shim_dim3 blockDim = {256, 1, 1};

// low 32 bits of a double's representation
static inline int __double2loint(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof u);
    return (int)(uint32_t)u;
}
