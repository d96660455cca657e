// contraction.h -- the inverse of the scene contraction, shared by tsdf.hip (its samples) and mesh.hip (its vertices) (device code).
// Both files are built with -ffp-contract=off: the operations below are the ones that run, every division the IEEE one.
#pragma once
#include "launch.h"

namespace sr {

// [REF extract_mesh_unbounded.uncontract, unnormalize] y in contracted space -> the world point uncontract(y) radius + center, in place:
// uncontract(y) = y for |y| < 1, else 1 / (2 - |y|) * (y / |y|) (a NaN norm takes the second branch, as torch.where does)
__device__ __forceinline__ void uncontract_to_world(float& x, float& y, float& z, const TsdfSpace& sp) {
    const float mag = __fsqrt_rn(x * x + y * y + z * z);
    if (!(mag < 1.f)) {
        const float k = __fdiv_rn(1.f, 2.f - mag);
        x = k * __fdiv_rn(x, mag); y = k * __fdiv_rn(y, mag); z = k * __fdiv_rn(z, mag);
    }
    x = x * sp.radius + sp.center[0]; y = y * sp.radius + sp.center[1]; z = z * sp.radius + sp.center[2];
}

}  // namespace sr
