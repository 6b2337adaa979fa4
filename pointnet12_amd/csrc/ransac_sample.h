// The integer sampler of the RANSAC entry points (plane.hip: rows of a cloud; corr_ransac.hip: rows of a pair list), in ONE place.
// The rule is the SAMPLER paragraph of include/pn2.h under "plane RANSAC"; tests/plane_ref.py restates it on Python integers.
#pragma once
#include <stdint.h>

constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

// row j of hypothesis h of cloud b among n rows
__device__ __forceinline__ int64_t ransac_sample(unsigned long long seed, int b, int h, int j, int n) {
    unsigned long long x = seed * kGolden + (((unsigned long long)b << 40) | ((unsigned long long)h << 8) | (unsigned long long)j);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (int64_t)(((x >> 32) * (unsigned long long)n) >> 32);
}
