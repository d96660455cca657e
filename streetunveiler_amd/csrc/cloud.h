// cloud.h -- the device helpers of the point-cloud searches (knn.hip, cluster.hip): both walk a cloud ordered by launch.h's CloudOrder
// steps, one wave64 per 64 curve-consecutive queries.  Both files are built with -ffp-contract=off: the operation order below is the one
// that runs.
#pragma once
#include "common.h"

namespace sr {

constexpr int kWave = 64;

__device__ __forceinline__ float wave_max(float v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// The squared distance of two points, in the operation order of the brute-force oracle and of the clustering predicate
__device__ __forceinline__ float dist2(const float4 a, const float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}
// A box (or a point: lo == hi) against a box, with the same operations on the gaps: a gap is no larger than the coordinate difference of
// any pair of points from the two, and subtraction, multiplication and addition of float32 are monotone, so a pair whose dist2 is below
// a bound has boxes whose gap2 is below it.  Needs no slack.  (An empty box is (FLT_MAX, -FLT_MAX): its gap2 is inf.)
__device__ __forceinline__ float gap2(const float4 alo, const float4 ahi, const float (&blo)[3], const float (&bhi)[3]) {
    const float gx = fmaxf(0.f, fmaxf(alo.x - bhi[0], blo[0] - ahi.x));
    const float gy = fmaxf(0.f, fmaxf(alo.y - bhi[1], blo[1] - ahi.y));
    const float gz = fmaxf(0.f, fmaxf(alo.z - bhi[2], blo[2] - ahi.z));
    return (gx * gx + gy * gy) + gz * gz;
}

}  // namespace sr
