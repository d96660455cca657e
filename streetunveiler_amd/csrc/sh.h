// sh.h -- the real spherical harmonics up to degree 3 as K1 / K8 and the SH gradient expansion use them: the basis, the colour it sums
// to, its adjoint, and the colour's derivative along the view direction  [REF utils/sh_utils.py:57-112].
//
// Coefficient k of degree band d lies in [d^2, (d+1)^2).  `deg` is the active degree: nothing in here reads or multiplies a
// coefficient of a higher band (0 * inf is NaN, and rows of fewer than 16 coefficients exist).  `deg` is uniform over a wave, so a
// band is one scalar branch.  Colours and adjoints are part of the bit-exact contract of preprocess.hip (-ffp-contract=off): every
// term is the product b[k] * value of ONE basis, the terms of a colour are added in ascending k.
#pragma once
#include "common.h"

namespace sr {

inline __device__ __constant__ float kSH_C0 = 0.28209479177387814f;
inline __device__ __constant__ float kSH_C1 = 0.4886025119029199f;
inline __device__ __constant__ float kSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                                   -1.0925484305920792f, 0.5462742152960396f};
inline __device__ __constant__ float kSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                                   0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                                   -0.5900435899266435f};

// b[k] = basis_k(x, y, z) for the unit direction (x, y, z); 0 above the active degree
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, float b[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = 0.f;
    b[0] = kSH_C0;
    if (deg > 0) {
        b[1] = -kSH_C1 * y; b[2] = kSH_C1 * z; b[3] = -kSH_C1 * x;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = kSH_C2[0] * xy; b[5] = kSH_C2[1] * yz; b[6] = kSH_C2[2] * (2.f * zz - xx - yy);
            b[7] = kSH_C2[3] * xz; b[8] = kSH_C2[4] * (xx - yy);
            if (deg > 2) {
                b[9] = kSH_C3[0] * y * (3.f * xx - yy);
                b[10] = kSH_C3[1] * xy * z;
                b[11] = kSH_C3[2] * y * (4.f * zz - xx - yy);
                b[12] = kSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                b[13] = kSH_C3[4] * x * (4.f * zz - xx - yy);
                b[14] = kSH_C3[5] * z * (xx - yy);
                b[15] = kSH_C3[6] * x * (xx - 3.f * yy);
            }
        }
    }
}

// The degree band of coefficient k.  A loop over ascending k that breaks at the first `sh_band(k) > deg` stops at (deg + 1)^2; unrolled,
// the compares of one band are one scalar branch.
constexpr __host__ __device__ int sh_band(int k) { return k < 1 ? 0 : k < 4 ? 1 : k < 9 ? 2 : 3; }

// The colour's terms of coefficients [K0, K1), b[k] * coeff[3 (k - K0) + c], added left to right onto res[c] (K0 == 0 starts the sum).
// K1 stages its rows through LDS one half at a time: <0, 8> on the first half, then <8, 16> on the second, with the one basis `b`.
template <int K0, int K1>
__device__ __forceinline__ void sh_to_rgb_range(int deg, const float b[16], const float* coeff, float res[3]) {
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        if (sh_band(k) > deg) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c] = k == 0 ? b[0] * coeff[c] : res[c] + b[k] * coeff[3 * (k - K0) + c];
    }
}
__device__ __forceinline__ void sh_to_rgb_lo(int deg, const float b[16], const float* lo, float res[3]) { sh_to_rgb_range<0, 8>(deg, b, lo, res); }
// ... and behind the last term: colour = SH + 0.5, clamped at 0 (flags recorded)
__device__ __forceinline__ void sh_to_rgb_hi(int deg, const float b[16], const float* hi, float res[3], float rgb[3], uint8_t& clamped) {
    sh_to_rgb_range<8, 16>(deg, b, hi, res);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = res[c] + 0.5f;
        if (r < 0.f) clamped |= (uint8_t)(1u << c);
        rgb[c] = fmaxf(r, 0.f);
    }
}

// The adjoint's terms b[k] * g[c] of the active coefficients: stored to dsh[3 k + c], or added onto it (the sum over the views of
// sh_gradient_expand_kernel: constant indices, dsh may be a register array).  Coefficients above the active degree are not touched.
template <bool kAccumulate, class RowOut>
__device__ __forceinline__ void sh_basis_adjoint_terms(int deg, const float b[16], RowOut dsh, const float g[3]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (sh_band(k) > deg) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) dsh[3 * k + c] = kAccumulate ? dsh[3 * k + c] + b[k] * g[c] : b[k] * g[c];
    }
}
// SH adjoint of a row of M coefficients in memory: dsh[3 k + c] = basis_k(dir) * g[c]; coefficients above the active degree get 0
template <class RowOut>
__device__ __forceinline__ void sh_basis_adjoint(int deg, int M, RowOut dsh, float x, float y, float z, const float g[3]) {
    float b[16];
    sh_basis(deg, x, y, z, b);
    sh_basis_adjoint_terms<false>(deg, b, dsh, g);
    const int used = (deg + 1) * (deg + 1);
    for (int k = used * 3; k < M * 3; ++k) dsh[k] = 0.f;
}

// d rgb[c] / d centre through the SH view direction, J[3 c + k] = ((d_c - dir (dir . d_c)) / len)[k] with d_c = d rgb[c] / d dir
// [REF the direction half of computeColorFromSH's backward, Appendix A.6].  K1 evaluates it next to the colour, from the SH row it
// holds anyway, so that K8 needs 36 B per Gaussian instead of reading the 192-B row again.  In the two halves of the row, like the
// colour: d[3 c + axis] accumulates d rgb[c] / d dir over coefficients 0..7, the second half adds 8..15, projects and scales.
// Not part of the bit-exact contract with the oracle (gradients are compared with a tolerance): contraction is allowed.
__device__ __forceinline__ void sh_dir_jacobian_lo(int deg, const float* lo, float x, float y, float z, float d[9]) {
#pragma clang fp contract(fast)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (deg > 0) {
            dx = -kSH_C1 * lo[9 + c]; dy = -kSH_C1 * lo[3 + c]; dz = kSH_C1 * lo[6 + c];
            if (deg > 1) {
                dx += (kSH_C2[0] * y) * lo[12 + c] + (-2.f * kSH_C2[2] * x) * lo[18 + c] + (kSH_C2[3] * z) * lo[21 + c];
                dy += (kSH_C2[0] * x) * lo[12 + c] + (kSH_C2[1] * z) * lo[15 + c] + (-2.f * kSH_C2[2] * y) * lo[18 + c];
                dz += (kSH_C2[1] * y) * lo[15 + c] + (4.f * kSH_C2[2] * z) * lo[18 + c] + (kSH_C2[3] * x) * lo[21 + c];
            }
        }
        d[3 * c] = dx; d[3 * c + 1] = dy; d[3 * c + 2] = dz;
    }
}
// The four polynomials of the degree-3 derivative.  They stand outside the contraction pragma: each operation is rounded on its own, so
// the derivative's bits do not depend on which of these products the compiler happens to share with sh_basis.
struct ShDirPolys { float xx_yy, px, py, pz; };
__device__ __forceinline__ ShDirPolys sh_dir_polys(float x, float y, float z) {
    const float xx = x * x, yy = y * y, zz = z * z;
    return {xx - yy, 4.f * zz - 3.f * xx - yy, 4.f * zz - 3.f * yy - xx, 2.f * zz - xx - yy};
}
__device__ __forceinline__ void sh_dir_jacobian_hi(int deg, const float* hi, float x, float y, float z, float len, const float d[9], float J[9]) {
#pragma clang fp contract(fast)
    const float inv_len = 1.f / len;
    const float xy = x * y, yz = y * z, xz = x * z;
    const ShDirPolys p = sh_dir_polys(x, y, z);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float dx = d[3 * c], dy = d[3 * c + 1], dz = d[3 * c + 2];
        if (deg > 1) {
            dx += (2.f * kSH_C2[4] * x) * hi[c];
            dy += (-2.f * kSH_C2[4] * y) * hi[c];
            if (deg > 2) {
                dx += (6.f * kSH_C3[0] * xy) * hi[3 + c] + (kSH_C3[1] * yz) * hi[6 + c] + (-2.f * kSH_C3[2] * xy) * hi[9 + c] +
                      (-6.f * kSH_C3[3] * xz) * hi[12 + c] + (kSH_C3[4] * p.px) * hi[15 + c] +
                      (2.f * kSH_C3[5] * xz) * hi[18 + c] + (3.f * kSH_C3[6] * p.xx_yy) * hi[21 + c];
                dy += (3.f * kSH_C3[0] * p.xx_yy) * hi[3 + c] + (kSH_C3[1] * xz) * hi[6 + c] + (kSH_C3[2] * p.py) * hi[9 + c] +
                      (-6.f * kSH_C3[3] * yz) * hi[12 + c] + (-2.f * kSH_C3[4] * xy) * hi[15 + c] + (-2.f * kSH_C3[5] * yz) * hi[18 + c] +
                      (-6.f * kSH_C3[6] * xy) * hi[21 + c];
                dz += (kSH_C3[1] * xy) * hi[6 + c] + (8.f * kSH_C3[2] * yz) * hi[9 + c] + (3.f * kSH_C3[3] * p.pz) * hi[12 + c] +
                      (8.f * kSH_C3[4] * xz) * hi[15 + c] + (kSH_C3[5] * p.xx_yy) * hi[18 + c];
            }
        }
        const float nd = (x * dx + y * dy) + z * dz;
        J[3 * c + 0] = (dx - x * nd) * inv_len; J[3 * c + 1] = (dy - y * nd) * inv_len; J[3 * c + 2] = (dz - z * nd) * inv_len;
    }
}

}  // namespace sr
