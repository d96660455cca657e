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
#include "abi.h"

namespace sr {

constexpr int kTsdfThreads = 256;

struct TsdfViewsDev {      // kernel parameters, by value
    const float* maps;     // device [V,H,W] depths (channels 1) or [V,H,W,4] (depth, r, g, b) records (channels 4)
    const float* full_proj;   // device [V,16]
    int V, H, W, channels;
};
struct TsdfGrid {          // sample (ix, iy, iz) = fmaf(index, step, lo) per axis; thread i is ix - ix0 = i / (ny nz), iy, iz
    float lo[3], step[3];
    int ny, nz, ix0;
};

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

// grid == nullptr: the n samples are read from `samples` [n,3]; rgb (with channels 4) and weight may be nullptr
static hipError_t launch_tsdf_fuse(const TsdfViewsDev& views, const TsdfSpace& space, const TsdfGrid* grid, int n, const float* samples, float* tsdf,
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

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks sr_tsdf_fuse and sr_tsdf_fuse_grid share -> the kernels' view of the arguments
static int tsdf_arguments(const SrTsdfViews* views, const SrTsdfSpace* space, long long n, const float* tsdf, const float* rgb, TsdfViewsDev* v,
                          TsdfSpace* sp) {
    if (!views || !space) return fail(SR_ERR_INVALID_ARGUMENT, "views / space is NULL");
    if (!views->maps) return fail(SR_ERR_INVALID_ARGUMENT, "maps is NULL");
    if (!views->full_proj) return fail(SR_ERR_INVALID_ARGUMENT, "full_proj is NULL");
    if (views->V < 1) return fail(SR_ERR_INVALID_ARGUMENT, "V = %d: at least one view", views->V);
    if (views->H < 2 || views->W < 2) return fail(SR_ERR_INVALID_ARGUMENT, "maps of %d x %d: H and W must be at least 2", views->H, views->W);
    if (views->channels != 1 && views->channels != 4) return fail(SR_ERR_INVALID_ARGUMENT, "channels = %d: 1 (depth) or 4 (depth, r, g, b)", views->channels);
    if ((uintptr_t)views->maps & (views->channels == 4 ? 15u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "maps is not %d-B aligned", 4 * views->channels);
    if ((uintptr_t)views->full_proj & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "full_proj is not 4-B aligned");
    if (!(space->voxel_size > 0.0)) return fail(SR_ERR_INVALID_ARGUMENT, "voxel_size = %g: must be positive", space->voxel_size);
    if (rgb && views->channels != 4) return fail(SR_ERR_INVALID_ARGUMENT, "rgb asked for, but the maps hold depths only (channels = 1)");
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n < 0");
    if (n >= (1ll << 31)) return fail(SR_ERR_UNSUPPORTED, "%lld samples in one call: fewer than 2^31 (split the call)", n);
    if (n > 0 && !tsdf) return fail(SR_ERR_INVALID_ARGUMENT, "tsdf is NULL");
    *v = TsdfViewsDev{views->maps, views->full_proj, views->V, views->H, views->W, views->channels};
    *sp = TsdfSpace{(float)(5.0 * space->voxel_size), space->contract ? 1 : 0, {space->center[0], space->center[1], space->center[2]}, space->radius};
    return SR_OK;
}

extern "C" {

int sr_tsdf_fuse(const SrTsdfViews* views, const SrTsdfSpace* space, int32_t n, const float* samples, float* tsdf, float* rgb, float* weight,
                 void* stream) {
    TsdfViewsDev v; TsdfSpace sp;
    if (int rc = tsdf_arguments(views, space, n, tsdf, rgb, &v, &sp)) return rc;
    if (n == 0) return SR_OK;
    if (!samples) return fail(SR_ERR_INVALID_ARGUMENT, "samples is NULL");
    SR_HIP(launch_tsdf_fuse(v, sp, nullptr, n, samples, tsdf, rgb, weight, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_tsdf_fuse_grid(const SrTsdfViews* views, const SrTsdfSpace* space, const int32_t* dims, const float* lo, const float* step,
                      int32_t ix_begin, int32_t ix_end, float* tsdf, float* rgb, float* weight, void* stream) {
    if (!dims || !lo || !step) return fail(SR_ERR_INVALID_ARGUMENT, "dims / lo / step is NULL");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(SR_ERR_INVALID_ARGUMENT, "dims %d x %d x %d: every axis holds at least one sample", dims[0], dims[1], dims[2]);
    if (ix_begin < 0 || ix_end < ix_begin || ix_end > dims[0]) return fail(SR_ERR_INVALID_ARGUMENT, "slab [%d, %d) is not inside [0, %d)", ix_begin, ix_end, dims[0]);
    if ((long long)dims[1] * dims[2] >= (1ll << 31)) return fail(SR_ERR_UNSUPPORTED, "one plane of %d x %d samples: fewer than 2^31", dims[1], dims[2]);
    const long long n = (long long)(ix_end - ix_begin) * dims[1] * dims[2];
    TsdfViewsDev v; TsdfSpace sp;
    if (int rc = tsdf_arguments(views, space, n, tsdf, rgb, &v, &sp)) return rc;
    if (n == 0) return SR_OK;
    const TsdfGrid g{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, dims[1], dims[2], ix_begin};
    SR_HIP(launch_tsdf_fuse(v, sp, &g, (int)n, nullptr, tsdf, rgb, weight, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
