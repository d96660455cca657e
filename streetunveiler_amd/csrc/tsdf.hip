// tsdf.hip -- the TSDF fusion of the rendered depth maps that the reference's mesh export evaluates on its marching-cubes samples
// (utils/mesh_utils.py:181-234: compute_sdf_perframe + compute_unbounded_tsdf) as one pass (include/surfel_raster.h states the semantics):
//   tsdf_fuse_kernel<RGB, GRID>   one thread per sample; the running tsdf, weight and colour stay in registers while the loop over the V
//                                 views runs inside the kernel.  RGB: the maps are [V,H,W,4] (depth, r, g, b) records, one 16-B load
//                                 per tap; else [V,H,W] depths.  GRID: the sample is generated from its index instead of read.
// The view matrices are read through a plain pointer indexed by the loop variable: wave-uniform, so they travel through the scalar
// cache, and there is no limit on V.  No atomics, no host read-back: equal inputs give equal bits.
// Built with -ffp-contract=off: the only fused operations are the fmaf()s written out below (the projection, the four taps and the
// grid coordinate), so all four instantiations evaluate one and the same expression per sample; every division is the IEEE one.
#include <cmath>

#include "contraction.h"
#include "launch.h"

namespace sr {

constexpr int kTsdfThreads = 256;

// [REF extract_mesh_unbounded.uncontract, unnormalize; compute_unbounded_tsdf lines 199-204] y in contracted space -> the world point
// and the truncation of the sample.  The "> 1" test is taken on the norm of the WORLD point, as the reference's line 201 does after
// line 200 has overwritten `samples`.
__device__ __forceinline__ float adaptive_trunc(float& x, float& y, float& z, const TsdfSpace& sp) {
    uncontract_to_world(x, y, z, sp);   // contraction.h
    const float norm = __fsqrt_rn(x * x + y * y + z * z);
    float trunc = sp.trunc;
    if (norm > 1.f) trunc *= __fdiv_rn(1.f, 2.f - fminf(norm, 1.9f));
    return trunc;
}

template <bool RGB> struct Tap;
template <> struct Tap<false> {
    float d;
    __device__ __forceinline__ void clear() { d = 0.f; }
    __device__ __forceinline__ void add(const float* __restrict__ maps, size_t at, float w) { d = fmaf(maps[at], w, d); }
};
template <> struct Tap<true> {
    float d, r, g, b;
    __device__ __forceinline__ void clear() { d = r = g = b = 0.f; }
    __device__ __forceinline__ void add(const float* __restrict__ maps, size_t at, float w) {
        const float4 t = reinterpret_cast<const float4*>(maps)[at];
        d = fmaf(t.x, w, d); r = fmaf(t.y, w, r); g = fmaf(t.z, w, g); b = fmaf(t.w, w, b);
    }
};

template <bool RGB, bool GRID>
__global__ __launch_bounds__(kTsdfThreads) void tsdf_fuse_kernel(const TsdfViewsDev views, const TsdfSpace space, const TsdfGrid grid, int n,
                                                                 const float* __restrict__ samples, float* __restrict__ out_tsdf,
                                                                 float* __restrict__ out_rgb, float* __restrict__ out_weight) {
    const unsigned i = blockIdx.x * (unsigned)kTsdfThreads + threadIdx.x;   // n < 2^31: no overflow
    if (i >= (unsigned)n) return;
    float x, y, z;
    if (GRID) {
        const unsigned plane = (unsigned)grid.ny * (unsigned)grid.nz;
        const unsigned ix = i / plane, rem = i - ix * plane, iy = rem / (unsigned)grid.nz, iz = rem - iy * (unsigned)grid.nz;
        x = fmaf((float)(ix + (unsigned)grid.ix0), grid.step[0], grid.lo[0]);
        y = fmaf((float)iy, grid.step[1], grid.lo[1]);
        z = fmaf((float)iz, grid.step[2], grid.lo[2]);
    } else {
        x = samples[3 * (size_t)i]; y = samples[3 * (size_t)i + 1]; z = samples[3 * (size_t)i + 2];
    }
    const float trunc = space.contract ? adaptive_trunc(x, y, z, space) : space.trunc;

    const int W = views.W, H = views.H;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const size_t plane = (size_t)H * (size_t)W;
    const float* __restrict__ maps = views.maps;
    float tsdf = 1.f, weight = 1.f, r = 0.f, g = 0.f, b = 0.f;   // [REF] the running average starts from a phantom observation of +1
    for (int v = 0; v < views.V; ++v) {
        const float* __restrict__ F = views.full_proj + 16 * (size_t)v;   // q = [x y z 1] F: row vector times matrix
        const float qx = fmaf(z, F[8], fmaf(y, F[4], fmaf(x, F[0], F[12])));
        const float qy = fmaf(z, F[9], fmaf(y, F[5], fmaf(x, F[1], F[13])));
        const float zc = fmaf(z, F[11], fmaf(y, F[7], fmaf(x, F[3], F[15])));
        const float px = __fdiv_rn(qx, zc), py = __fdiv_rn(qy, zc);
        if (!(px > -1.f && px < 1.f && py > -1.f && py < 1.f && zc > 0.f)) continue;   // a NaN is false: masked out, nothing fetched
        // grid_sample(bilinear, align_corners=True); with the mask passed 0 <= fx <= W - 1, so border padding changes nothing
        const float fx = __fdiv_rn(px + 1.f, 2.f) * wm1, fy = __fdiv_rn(py + 1.f, 2.f) * hm1;
        const float x0f = floorf(fx), y0f = floorf(fy);
        const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
        const float ex = (x0f + 1.f) - fx, ey = (y0f + 1.f) - fy, dx = fx - x0f, dy = fy - y0f;
        // every in-bounds tap is multiplied in, a zero weight included (a non-finite pixel poisons the sample as in torch); a tap
        // whose index is out of bounds is not read: px = 1 - 2^-24 gives fx == W - 1 exactly, and x1 == W
        const bool inx0 = x0 >= 0 && x0 < W, inx1 = x1 >= 0 && x1 < W, iny0 = y0 >= 0 && y0 < H, iny1 = y1 >= 0 && y1 < H;
        const size_t base = (size_t)v * plane;
        Tap<RGB> tap;
        tap.clear();
        if (inx0 && iny0) tap.add(maps, base + (size_t)y0 * W + x0, ex * ey);   // nw
        if (inx1 && iny0) tap.add(maps, base + (size_t)y0 * W + x1, dx * ey);   // ne
        if (inx0 && iny1) tap.add(maps, base + (size_t)y1 * W + x0, ex * dy);   // sw
        if (inx1 && iny1) tap.add(maps, base + (size_t)y1 * W + x1, dx * dy);   // se
        const float sdf = tap.d - zc;
        if (!(sdf > -trunc)) continue;
        const float s = fminf(fmaxf(__fdiv_rn(sdf, trunc), -1.f), 1.f);   // (sdf is no NaN here)
        const float wp = weight + 1.f;
        tsdf = __fdiv_rn(tsdf * weight + s, wp);
        if constexpr (RGB) {
            r = __fdiv_rn(r * weight + tap.r, wp);
            g = __fdiv_rn(g * weight + tap.g, wp);
            b = __fdiv_rn(b * weight + tap.b, wp);
        }
        weight = wp;
    }
    out_tsdf[i] = tsdf;
    if constexpr (RGB) if (out_rgb) { out_rgb[3 * (size_t)i] = r; out_rgb[3 * (size_t)i + 1] = g; out_rgb[3 * (size_t)i + 2] = b; }
    if (out_weight) out_weight[i] = weight;
}

hipError_t launch_tsdf_fuse(const TsdfViewsDev& views, const TsdfSpace& space, const TsdfGrid* grid, int n, const float* samples, float* tsdf,
                            float* rgb, float* weight, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 blocks((unsigned)(((size_t)n + kTsdfThreads - 1) / kTsdfThreads)), threads(kTsdfThreads);
    const TsdfGrid g = grid ? *grid : TsdfGrid{};
    const bool colour = views.channels == 4;
    if (colour && grid) hipLaunchKernelGGL((tsdf_fuse_kernel<true, true>), blocks, threads, 0, s, views, space, g, n, samples, tsdf, rgb, weight);
    else if (colour) hipLaunchKernelGGL((tsdf_fuse_kernel<true, false>), blocks, threads, 0, s, views, space, g, n, samples, tsdf, rgb, weight);
    else if (grid) hipLaunchKernelGGL((tsdf_fuse_kernel<false, true>), blocks, threads, 0, s, views, space, g, n, samples, tsdf, rgb, weight);
    else hipLaunchKernelGGL((tsdf_fuse_kernel<false, false>), blocks, threads, 0, s, views, space, g, n, samples, tsdf, rgb, weight);
    return hipGetLastError();
}

}  // namespace sr
