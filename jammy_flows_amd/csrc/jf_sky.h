// What the sky kernels share (sky_kernels.hip, sky_refine_kernels.hip): the NUNIQ id arithmetic and the binary search of an ascending row.
#pragma once
#include <stdint.h>

#include "../../include/jammy_hip_sky.h"

namespace jf {
namespace sky {

constexpr int MAX_ORDER = JF_SKY_MAX_ORDER;

// NUNIQ id -> (order, pixel); false for padding (ids below 4, hence -1) and ids beyond order 29
__host__ __device__ __forceinline__ bool decode_uniq(int64_t uniq, int& order, int64_t& pix) {
    if (uniq < 4) return false;
    const int msb = 63 - __builtin_clzll((unsigned long long)uniq);
    order = (msb - 2) >> 1;
    pix = uniq - ((int64_t)4 << (2 * order));
    return order <= MAX_ORDER;
}

// first index in [0, n) of the ascending row whose value is >= key (n when there is none)
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ row, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace sky
}  // namespace jf
