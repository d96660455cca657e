// unveil.hip -- the frame masks of the unveiling stage (include/surfel_raster.h states the semantics):
//   per point  [REF scene/__init__.py:217-312, inpainting_pipeline/1_selection/1_instance_visualization.py:85-100]
//     points_in_frame_kernel      one thread per point, one camera: the in-frame flag (and its word for the compaction's scan)
//     points_emit_kernel          the admitted points' (pix.x, pix.y) int64 and depth, at the scanned offsets: ascending point index
//     frame_visibility_kernel     a block holds kVisRows x 256 points in registers and walks the F frames; per frame the block's count and
//                                 depth sum are folded in a fixed order (reduce.h) into one partial per (frame, block)
//     frame_visibility_finalize_kernel   one workgroup per frame adds the partials (reduce.h)
//     semantic_mask_kernel        one thread per point, the loop over the frames inside; a thread leaves the loop once its point is set
//   per pixel  [REF inpainting_pipeline/utils.py:17-30, 2_condition_preparation/2_generate_inpainted_mask.py:111-159,
//               3_reoptimization/1_optimization.py:115-187]
//     dilate_kernel<Source>       the k x k dilation of a predicate the block evaluates itself: a mask byte, |a - b| > threshold, or
//                                 ~(sum |a - b| < eps) & mask.  Bit-packed rows in the LDS (below).
//     conditions_kernel           the five uint8 images of a frame, one thread per pixel
//
// The dilation.  A block owns a tile of 64 x kDilateRows output pixels.  A wave evaluates the predicate on 64 consecutive pixels of a
// row and its ballot IS the packed row word; per staged row three words are kept (the 64 columns left of the tile, the tile's, the 64
// right of it -- of the outer two only the lanes within the window's reach evaluate anything, the others load nothing).  One thread per
// staged row then ORs the k horizontal shifts of its 192 bits into one word, one thread per output row ORs the k staged rows, and the
// block writes its bytes.  Per tile (kDilateRows + k - 1) x (64 + k - 1) predicate evaluations, 2 k 64-bit ORs per row, no float ever
// stored.  The window is [-(k/2), k - 1 - k/2] in both axes; pixels outside the image are never read and contribute nothing.
//
// Every index is tested before it is used: a pixel index against [0, H) x [0, W), a compaction offset against n, a semantic-map index
// against [0, Hm) x [0, Wm).  Integer atomics only (the out-of-range counter); the float sums are fixed-order folds: equal inputs give
// equal bits.  Built with -ffp-contract=off: the projection, the composites and the quantisation are the float32 operations written
// below, one rounding each, as the stock-torch lines they restate evaluate them.
#include <cmath>

#include "abi.h"
#include "reduce.h"

namespace sr {

constexpr int kUnveilCamFloats = 24;   // a camera row: w2c rows 0..2 (12), K (9), max_z (+inf: none), reso_scale (0: none), one unused
constexpr int kDilateRows = 32;        // output rows of a dilation tile (64 columns wide); the tile rows are grid.y: H <= 32 * 65535
struct UnveilSemantic {    // a kernel parameter, by value: device pointers
    int P, F, Hm, Wm;
    uint32_t remain_bit;   // bits 0..30
    const float* xyz;      // [P,3]
    const float* cams;     // [F,kUnveilCamFloats]
    const int32_t* hw;     // [F,2] = (h, w)
    const uint8_t* maps;   // [F,Hm,Wm] labels
};
struct UnveilConditions {  // a kernel parameter, by value: device pointers; the images are [C,H,W] float32, the outputs [H,W,C] uint8
    int H, W;
    const float *full_render, *full_alpha, *background_render, *background_alpha, *background_depth, *background_normal, *sky;
    uint8_t *original_rgb, *inpainted_rgb, *empty_opacity, *inpainted_depth, *inpainted_normal;
};

constexpr int kUnveilThreads = 256;
constexpr int kVisRows = 8;                                 // points a thread of frame_visibility_kernel holds
constexpr int kVisChunk = kVisRows * kReduceThreads;         // 2048 points a block
constexpr int kDilateMaxK = 31;
constexpr int kDilateStaged = kDilateRows + kDilateMaxK - 1;

// ---- the predicate ---------------------------------------------------------------------------------------------------------------------
struct FrameHit {
    bool in;
    float depth;      // cam.z
    float u, v;       // pix (only meaningful where in)
};

// cams + kUnveilCamFloats f: {w2c rows 0..2 (12), K (9), max_z (+inf: none), reso_scale (0: none), unused}; hw + 2 f: {h, w}
__device__ __forceinline__ FrameHit project_point(const float* __restrict__ cam, int h, int w, float x, float y, float z) {
    const float cx = cam[0] * x + cam[1] * y + cam[2] * z + cam[3];
    const float cy = cam[4] * x + cam[5] * y + cam[6] * z + cam[7];
    // the depth is an output (and what depth_sum adds): the float64 expression rounded once, so it is within half an ulp of the float64
    // checker's whichever way a float32 implementation orders the sum.  (Three exact products and three float64 additions.)
    const float cz = (float)((double)cam[8] * (double)x + (double)cam[9] * (double)y + (double)cam[10] * (double)z + (double)cam[11]);
    const float px = cam[12] * cx + cam[13] * cy + cam[14] * cz;
    const float py = cam[15] * cx + cam[16] * cy + cam[17] * cz;
    const float pw = cam[18] * cx + cam[19] * cy + cam[20] * cz;
    const float u = __fdiv_rn(px, pw), v = __fdiv_rn(py, pw);
    FrameHit hit;
    // strict, and false for a NaN; an infinite coordinate gives an infinite or NaN pix and is tested for on its own as well
    hit.in = u < (float)w && u > 0.f && v < (float)h && v > 0.f && cz > 0.f && cz < cam[21] && isfinite(x) && isfinite(y) && isfinite(z);
    hit.depth = cz;
    hit.u = u;
    hit.v = v;
    return hit;
}

// trunc(pix), then trunc(trunc(pix) / reso_scale) in float32 where a scale is given.  0 < pix < 2^31 for an admitted point; the scaled
// value is clamped into what an int64 holds before it is converted.
__device__ __forceinline__ long long pixel_coord(float pix, float reso) {
    float q = truncf(pix);
    if (reso > 0.f) q = fminf(fmaxf(truncf(__fdiv_rn(q, reso)), -9.0e18f), 9.0e18f);
    return (long long)q;
}

// ---- one camera: flags, compaction ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kUnveilThreads) void points_in_frame_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ cam,
                                                                         const int32_t* __restrict__ hw, uint8_t* __restrict__ mask,
                                                                         uint32_t* __restrict__ flags) {
    const unsigned i = blockIdx.x * (unsigned)kUnveilThreads + threadIdx.x;   // P < 2^31: no overflow
    if (i >= (unsigned)P) return;
    const FrameHit hit = project_point(cam, hw[0], hw[1], xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    mask[i] = hit.in ? 1 : 0;
    if (flags) flags[i] = hit.in ? 1u : 0u;
}

// offsets: the exclusive scan of the flags; n: the number of rows the caller allocated (the scan's total, read back)
__global__ __launch_bounds__(kUnveilThreads) void points_emit_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ cam,
                                                                     const int32_t* __restrict__ hw, const uint32_t* __restrict__ offsets, uint32_t n,
                                                                     long long* __restrict__ pix, float* __restrict__ depth) {
    const unsigned i = blockIdx.x * (unsigned)kUnveilThreads + threadIdx.x;
    if (i >= (unsigned)P) return;
    const FrameHit hit = project_point(cam, hw[0], hw[1], xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    if (!hit.in) return;
    const uint32_t at = offsets[i];
    if (at >= n) return;
    pix[2 * (size_t)at] = pixel_coord(hit.u, cam[22]);
    pix[2 * (size_t)at + 1] = pixel_coord(hit.v, cam[22]);
    depth[at] = hit.depth;
}

// ---- points x frames: counts and depth sums -------------------------------------------------------------------------------------------
// partials[(f n_blocks + b) 2 + {0, 1}] = the count (exact in a double) and the depth sum of block b's points in frame f
__global__ __launch_bounds__(kReduceThreads) void frame_visibility_kernel(int P, int F, const float* __restrict__ xyz, const float* __restrict__ cams,
                                                                          const int32_t* __restrict__ hw, double* __restrict__ partials) {
    __shared__ double red[kReduceThreads];
    float px[kVisRows], py[kVisRows], pz[kVisRows];
    const unsigned base = blockIdx.x * (unsigned)kVisChunk;   // P < 2^31 and base < P: base + 2047 does not overflow 32 bits
#pragma unroll
    for (int r = 0; r < kVisRows; ++r) {
        const unsigned i = base + (unsigned)r * kReduceThreads + threadIdx.x;
        const bool valid = i < (unsigned)P;
        px[r] = valid ? xyz[3 * (size_t)i] : NAN;      // a NaN is in no frame
        py[r] = valid ? xyz[3 * (size_t)i + 1] : NAN;
        pz[r] = valid ? xyz[3 * (size_t)i + 2] : NAN;
    }
    for (int f = 0; f < F; ++f) {
        const float* cam = cams + (size_t)f * kUnveilCamFloats;
        const int h = hw[2 * (size_t)f], w = hw[2 * (size_t)f + 1];
        double count = 0.0, sum = 0.0;
#pragma unroll
        for (int r = 0; r < kVisRows; ++r) {
            const FrameHit hit = project_point(cam, h, w, px[r], py[r], pz[r]);
            if (hit.in) { count += 1.0; sum += (double)hit.depth; }
        }
        const double block_count = block_sum(count, red);
        const double block_depth = block_sum(sum, red);
        if (threadIdx.x == 0) {
            const size_t at = 2 * ((size_t)f * gridDim.x + blockIdx.x);
            partials[at] = block_count;
            partials[at + 1] = block_depth;
        }
    }
}

__global__ __launch_bounds__(kReduceThreads) void frame_visibility_finalize_kernel(const double* __restrict__ partials, int n_blocks,
                                                                                   long long* __restrict__ count, double* __restrict__ depth_sum) {
    __shared__ double red[kReduceThreads];
    double sums[2];
    finalize_sums<2>(partials + 2 * (size_t)blockIdx.x * (size_t)n_blocks, n_blocks, red, sums);
    if (threadIdx.x == 0) {
        count[blockIdx.x] = (long long)sums[0];
        depth_sum[blockIdx.x] = sums[1];
    }
}

// ---- the semantic mask of the cloud over all frames -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kUnveilThreads) void semantic_mask_kernel(const UnveilSemantic a, uint8_t* __restrict__ mask,
                                                                       unsigned long long* __restrict__ n_out_of_range) {
    const unsigned i = blockIdx.x * (unsigned)kUnveilThreads + threadIdx.x;
    if (i >= (unsigned)a.P) return;
    const float x = a.xyz[3 * (size_t)i], y = a.xyz[3 * (size_t)i + 1], z = a.xyz[3 * (size_t)i + 2];
    const size_t plane = (size_t)a.Hm * (size_t)a.Wm;
    unsigned outside = 0u;
    bool set = false;
    for (int f = 0; f < a.F && !set; ++f) {
        const float* cam = a.cams + (size_t)f * kUnveilCamFloats;
        const FrameHit hit = project_point(cam, a.hw[2 * (size_t)f], a.hw[2 * (size_t)f + 1], x, y, z);
        if (!hit.in) continue;
        const long long mx = pixel_coord(hit.u, cam[22]), my = pixel_coord(hit.v, cam[22]);
        if (mx < 0 || mx >= a.Wm || my < 0 || my >= a.Hm) { ++outside; continue; }   // not read: matches nothing, counted
        const uint32_t label = a.maps[(size_t)f * plane + (size_t)my * (size_t)a.Wm + (size_t)mx];
        set = label < 31u && ((1u << label) & a.remain_bit) != 0u;                    // a label of 31 or more matches nothing
    }
    mask[i] = set ? 1 : 0;
    if (outside) atomicAdd(n_out_of_range, (unsigned long long)outside);
}

// ---- the dilation ---------------------------------------------------------------------------------------------------------------------
struct MaskSource {          // a mask byte: set where it is not 0
    const uint8_t* mask;
    __device__ __forceinline__ bool operator()(size_t at, size_t) const { return mask[at] != 0; }
};
struct AlphaDiffSource {     // |a - b| > threshold; a NaN difference is not set
    const float *a, *b;
    float threshold;
    __device__ __forceinline__ bool operator()(size_t at, size_t) const { return fabsf(a[at] - b[at]) > threshold; }
};
struct RefillSource {        // ~(sum over the channels of |a - b| < eps) & mask; a NaN sum is set
    const float *a, *b;
    const uint8_t* mask;
    float eps;
    int C;
    __device__ __forceinline__ bool operator()(size_t at, size_t plane) const {
        if (mask[at] == 0) return false;
        float sum = fabsf(a[at] - b[at]);
        for (int c = 1; c < C; ++c) sum += fabsf(a[at + (size_t)c * plane] - b[at + (size_t)c * plane]);
        return !(sum < eps);
    }
};

template <class Source>
__global__ __launch_bounds__(kUnveilThreads) void dilate_kernel(int H, int W, int k, const Source source, uint8_t* __restrict__ out) {
    __shared__ unsigned long long s_bits[kDilateStaged][3];   // staged row r = image row y0 - up + r: the words left of, of and right of the tile
    __shared__ unsigned long long s_rows[kDilateStaged];      // the same rows, dilated horizontally: the tile's 64 columns
    __shared__ unsigned long long s_out[kDilateRows];
    const int up = k / 2, down = k - 1 - k / 2;               // the window's reach: up = left, down = right; both <= 15
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * kDilateRows;
    const int staged = kDilateRows + up + down;               // <= kDilateStaged
    const size_t plane = (size_t)H * (size_t)W;
    for (int item = wave; item < 3 * staged; item += kUnveilThreads / 64) {   // wave-uniform bounds: all 64 lanes reach the ballot
        const int r = item / 3, j = item - 3 * r;
        const int y = y0 - up + r, x = x0 + (j - 1) * 64 + lane;
        const bool reach = j == 1 || (j == 0 && lane >= 64 - up) || (j == 2 && lane < down);
        bool bit = false;
        if (reach && y >= 0 && y < H && x >= 0 && x < W) bit = source((size_t)y * (size_t)W + (size_t)x, plane);
        const unsigned long long word = ballot64(bit);
        if (lane == 0) s_bits[r][j] = word;
    }
    __syncthreads();
    if ((int)threadIdx.x < staged) {
        const unsigned long long left = s_bits[threadIdx.x][0], centre = s_bits[threadIdx.x][1], right = s_bits[threadIdx.x][2];
        unsigned long long row = centre;
        for (int d = 1; d <= down; ++d) row |= (centre >> d) | (right << (64 - d));   // column x + d
        for (int d = 1; d <= up; ++d) row |= (centre << d) | (left >> (64 - d));      // column x - d
        s_rows[threadIdx.x] = row;
    }
    __syncthreads();
    if ((int)threadIdx.x < kDilateRows) {
        unsigned long long word = 0ull;
        for (int r = 0; r <= up + down; ++r) word |= s_rows[threadIdx.x + r];         // image rows y - up .. y + down
        s_out[threadIdx.x] = word;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < kDilateRows * 64; p += kUnveilThreads) {
        const int row = p >> 6, col = p & 63;
        const int y = y0 + row, x = x0 + col;
        if (y < H && x < W) out[(size_t)y * (size_t)W + (size_t)x] = (uint8_t)((s_out[row] >> col) & 1ull);
    }
}

template <class Source>
static hipError_t launch_dilate(int H, int W, int k, const Source& source, uint8_t* out, hipStream_t s) {
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + kDilateRows - 1) / kDilateRows));
    hipLaunchKernelGGL(dilate_kernel<Source>, grid, dim3(kUnveilThreads), 0, s, H, W, k, source, out);
    return hipGetLastError();
}

// ---- the condition images -------------------------------------------------------------------------------------------------------------
// torchvision's save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two roundings, then the truncation; a NaN becomes 0
__device__ __forceinline__ uint8_t quantise(float x) {
    const float v = x * 255.f + 0.5f;                // (-ffp-contract=off: a product, then a sum)
    return (uint8_t)fminf(fmaxf(v, 0.f), 255.f);     // fmaxf(NaN, 0) = 0
}
__device__ __forceinline__ float clamp01(float x) { return x != x ? x : fminf(fmaxf(x, 0.f), 1.f); }   // torch.clamp keeps a NaN

__global__ __launch_bounds__(kUnveilThreads) void conditions_kernel(const UnveilConditions a) {
    const size_t n = (size_t)a.H * (size_t)a.W;
    const size_t i = (size_t)blockIdx.x * kUnveilThreads + threadIdx.x;
    if (i >= n) return;
    const float alpha = a.full_alpha[i];
    const float t = 1.f - alpha;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sky = a.sky[i + (size_t)c * n] * t;
        a.original_rgb[3 * i + c] = quantise(a.full_render[i + (size_t)c * n] + sky);
        a.inpainted_rgb[3 * i + c] = quantise(a.background_render[i + (size_t)c * n] + sky);      // the FULL alpha, as the reference
        a.inpainted_normal[3 * i + c] = quantise(clamp01(a.background_normal[i + (size_t)c * n] * 0.5f + 0.5f));
    }
    a.empty_opacity[i] = quantise(alpha - a.background_alpha[i]);
    float d = __fdiv_rn(1.f, a.background_depth[i]);
    if (isinf(d)) d = 0.f;
    a.inpainted_depth[i] = quantise(clamp01(d));
}

// ---- the launchers --------------------------------------------------------------------------------------------------------------------
static dim3 unveil_grid(size_t n) { return dim3((unsigned)((n + kUnveilThreads - 1) / kUnveilThreads)); }
static int visibility_blocks(int P) { return (int)(((long long)P + kVisChunk - 1) / kVisChunk); }

// offsets: one word a point + the chunk sums of its scan;  partials: two doubles per (frame, block of kVisChunk points)
struct UnveilLayout {
    size_t offsets, chunks, partials, total;
};
static UnveilLayout unveil_layout(int P, int F) {
    UnveilLayout L;
    Carver c;
    const size_t p = P > 0 ? P : 1, f = F > 0 ? F : 1;
    L.offsets = c.take(4 * p);
    L.chunks = c.take(4 * scan_in_place_chunk_words((uint32_t)p));
    L.partials = c.take(16 * f * (size_t)visibility_blocks((int)p));
    L.total = c.off;
    return L;
}
static size_t unveil_workspace_bytes(int P, int F) { return unveil_layout(P, F).total; }

// P >= 1.  count == nullptr: the mask alone; else the offsets of the admitted points are left in the workspace and *count (device) = n
static hipError_t points_in_frame(int P, const float* xyz, const float* cam, const int32_t* hw, uint8_t* mask, void* ws, uint32_t* count, hipStream_t s) {
    uint32_t* offsets = count ? at<uint32_t>(ws, unveil_layout(P, 1).offsets) : nullptr;
    hipLaunchKernelGGL(points_in_frame_kernel, unveil_grid(P), dim3(kUnveilThreads), 0, s, P, xyz, cam, hw, mask, offsets);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !count) return e;
    return exclusive_scan_in_place(offsets, (uint32_t)P, at<uint32_t>(ws, unveil_layout(P, 1).chunks), count, s);
}

// after points_in_frame with a count on the same points, camera and workspace; n >= 1 rows
static hipError_t points_in_frame_emit(int P, const float* xyz, const float* cam, const int32_t* hw, const void* ws, uint32_t n, int64_t* pix, float* depth,
                                hipStream_t s) {
    const uint32_t* offsets = at<const uint32_t>(const_cast<void*>(ws), unveil_layout(P, 1).offsets);
    hipLaunchKernelGGL(points_emit_kernel, unveil_grid(P), dim3(kUnveilThreads), 0, s, P, xyz, cam, hw, offsets, n, reinterpret_cast<long long*>(pix), depth);
    return hipGetLastError();
}

// P, F >= 1
static hipError_t frame_visibility(int P, int F, const float* xyz, const float* cams, const int32_t* hw, void* ws, int64_t* count, double* depth_sum,
                            hipStream_t s) {
    double* partials = at<double>(ws, unveil_layout(P, F).partials);
    const int n_blocks = visibility_blocks(P);
    hipLaunchKernelGGL(frame_visibility_kernel, dim3(n_blocks), dim3(kReduceThreads), 0, s, P, F, xyz, cams, hw, partials);
    hipLaunchKernelGGL(frame_visibility_finalize_kernel, dim3(F), dim3(kReduceThreads), 0, s, partials, n_blocks, reinterpret_cast<long long*>(count),
                       depth_sum);
    return hipGetLastError();
}

// a.P, a.F >= 1; n_out_of_range: device [1]
static hipError_t semantic_mask_of_points(const UnveilSemantic& a, uint8_t* mask, uint64_t* n_out_of_range, hipStream_t s) {
    hipError_t e = hipMemsetAsync(n_out_of_range, 0, 8, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(semantic_mask_kernel, unveil_grid(a.P), dim3(kUnveilThreads), 0, s, a, mask, reinterpret_cast<unsigned long long*>(n_out_of_range));
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks the per-point sr_* calls share; *work = 0 where there is no point or no frame
static int unveil_point_arguments(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, bool* work) {
    if (P < 0 || F < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P %d / F %d is negative", P, F);
    *work = P > 0 && F > 0;
    if (!*work) return SR_OK;
    if (!xyz || !cams || !hw) return fail(SR_ERR_INVALID_ARGUMENT, "xyz / cams / hw is NULL");
    if (((uintptr_t)xyz | (uintptr_t)cams | (uintptr_t)hw) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "xyz / cams / hw is not 4-B aligned");
    return SR_OK;
}

// the checks the per-pixel sr_* calls share
static int unveil_image_arguments(int32_t H, int32_t W, int32_t k) {
    if (H < 1 || W < 1) return fail(SR_ERR_INVALID_ARGUMENT, "an image of %d x %d: H and W must be at least 1", H, W);
    if ((long long)H * W > 0x7FFFFFFFll) return fail(SR_ERR_UNSUPPORTED, "an image of %d x %d: H W must fit in int32", H, W);
    // a tile is 64 x kDilateRows pixels: the tile rows are the launch's grid.y, and a tile's halo reaches 64 columns past its own
    if (H > kDilateRows * 65535) return fail(SR_ERR_UNSUPPORTED, "an image of %d rows: at most %d", H, kDilateRows * 65535);
    if (W > 0x7FFFFFFF - 128) return fail(SR_ERR_UNSUPPORTED, "an image of %d columns: at most %d", W, 0x7FFFFFFF - 128);
    if (k < 1 || k > 31) return fail(SR_ERR_INVALID_ARGUMENT, "k = %d not in 1..31", k);
    return SR_OK;
}

extern "C" {

size_t sr_unveil_workspace_bytes(int32_t P, int32_t F) {
    if (P < 0 || F < 0) return 0;
    return unveil_workspace_bytes(P, F);
}

int sr_points_in_frame(int32_t P, const float* xyz, const float* cam, const int32_t* hw, uint8_t* mask, void* workspace, size_t workspace_bytes,
                       uint32_t* count, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, 1, xyz, cam, hw, &work)) return rc;
    if ((uintptr_t)count & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "count is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {
        if (count) SR_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
        return SR_OK;
    }
    if (!mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    if (count) if (int rc = check_workspace(workspace, workspace_bytes, unveil_workspace_bytes(P, 1))) return rc;
    SR_HIP(points_in_frame(P, xyz, cam, hw, mask, workspace, count, s));
    return SR_OK;
}

int sr_points_in_frame_emit(int32_t P, const float* xyz, const float* cam, const int32_t* hw, void* workspace, size_t workspace_bytes, int32_t n,
                            int64_t* pix, float* depth, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, 1, xyz, cam, hw, &work)) return rc;
    if (n < 0 || n > P) return fail(SR_ERR_INVALID_ARGUMENT, "n = %d: not in 0..P = %d", n, P);
    if (n == 0) return SR_OK;
    if (int rc = check_workspace(workspace, workspace_bytes, unveil_workspace_bytes(P, 1))) return rc;
    if (!pix || !depth) return fail(SR_ERR_INVALID_ARGUMENT, "pix / depth is NULL");
    if (((uintptr_t)pix & 7u) || ((uintptr_t)depth & 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "pix is not 8-B or depth not 4-B aligned");
    SR_HIP(points_in_frame_emit(P, xyz, cam, hw, workspace, (uint32_t)n, pix, depth, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_frame_visibility(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, void* workspace, size_t workspace_bytes,
                        int64_t* count, double* depth_sum, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, F, xyz, cams, hw, &work)) return rc;
    if (F == 0) return SR_OK;
    if (!count || !depth_sum) return fail(SR_ERR_INVALID_ARGUMENT, "count / depth_sum is NULL");
    if (((uintptr_t)count | (uintptr_t)depth_sum) & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "count / depth_sum is not 8-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {   // no point: every count and sum is 0 (all bits zero)
        SR_HIP(hipMemsetAsync(count, 0, sizeof(int64_t) * (size_t)F, s));
        SR_HIP(hipMemsetAsync(depth_sum, 0, sizeof(double) * (size_t)F, s));
        return SR_OK;
    }
    if (int rc = check_workspace(workspace, workspace_bytes, unveil_workspace_bytes(P, F))) return rc;
    SR_HIP(frame_visibility(P, F, xyz, cams, hw, workspace, count, depth_sum, s));
    return SR_OK;
}

int sr_semantic_mask_of_points(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, const uint8_t* maps, int32_t Hm,
                               int32_t Wm, uint32_t remain_bit, uint8_t* mask, uint64_t* n_out_of_range, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, F, xyz, cams, hw, &work)) return rc;
    if (Hm < 1 || Wm < 1) return fail(SR_ERR_INVALID_ARGUMENT, "maps of %d x %d: Hm and Wm must be at least 1", Hm, Wm);
    if (!n_out_of_range) return fail(SR_ERR_INVALID_ARGUMENT, "n_out_of_range is NULL");
    if ((uintptr_t)n_out_of_range & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "n_out_of_range is not 8-B aligned");
    if (P > 0 && !mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {   // no frame sets anything
        SR_HIP(hipMemsetAsync(n_out_of_range, 0, sizeof(uint64_t), s));
        if (P > 0) SR_HIP(hipMemsetAsync(mask, 0, (size_t)P, s));
        return SR_OK;
    }
    if (!maps) return fail(SR_ERR_INVALID_ARGUMENT, "maps is NULL");
    const UnveilSemantic a{P, F, Hm, Wm, remain_bit & 0x7FFFFFFFu, xyz, cams, hw, maps};
    SR_HIP(semantic_mask_of_points(a, mask, n_out_of_range, s));
    return SR_OK;
}

int sr_dilate_mask(int32_t H, int32_t W, int32_t k, const uint8_t* mask, uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!mask || !out) return fail(SR_ERR_INVALID_ARGUMENT, "mask / out is NULL");
    if (mask == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the mask: a tile reads its neighbours' pixels");
    SR_HIP(launch_dilate(H, W, k, MaskSource{mask}, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_instance_pixel_mask(int32_t H, int32_t W, const float* alpha_a, const float* alpha_b, float threshold, int32_t k, uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!alpha_a || !alpha_b || !out) return fail(SR_ERR_INVALID_ARGUMENT, "alpha_a / alpha_b / out is NULL");
    if (((uintptr_t)alpha_a | (uintptr_t)alpha_b) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "alpha_a / alpha_b is not 4-B aligned");
    if (threshold != threshold) return fail(SR_ERR_INVALID_ARGUMENT, "threshold is NaN");
    SR_HIP(launch_dilate(H, W, k, AlphaDiffSource{alpha_a, alpha_b, threshold}, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_refill_mask(int32_t H, int32_t W, int32_t C, const float* render_a, const float* render_b, const uint8_t* mask, float eps, int32_t k,
                   uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (C < 1 || C > 16) return fail(SR_ERR_UNSUPPORTED, "C = %d channels: 1..16", C);
    if (!render_a || !render_b || !mask || !out) return fail(SR_ERR_INVALID_ARGUMENT, "render_a / render_b / mask / out is NULL");
    if (mask == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the mask: a tile reads its neighbours' pixels");
    if (((uintptr_t)render_a | (uintptr_t)render_b) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "render_a / render_b is not 4-B aligned");
    if (eps != eps) return fail(SR_ERR_INVALID_ARGUMENT, "eps is NaN");
    SR_HIP(launch_dilate(H, W, k, RefillSource{render_a, render_b, mask, eps, C}, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_inpaint_conditions(int32_t H, int32_t W, const float* full_render, const float* full_alpha, const float* background_render,
                          const float* background_alpha, const float* background_depth, const float* background_normal, const float* sky,
                          float threshold, int32_t k, uint8_t* mask, uint8_t* original_rgb, uint8_t* inpainted_rgb, uint8_t* empty_opacity,
                          uint8_t* inpainted_depth, uint8_t* inpainted_normal, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!full_render || !full_alpha || !background_render || !background_alpha || !background_depth || !background_normal || !sky)
        return fail(SR_ERR_INVALID_ARGUMENT, "an input image is NULL");
    if (((uintptr_t)full_render | (uintptr_t)full_alpha | (uintptr_t)background_render | (uintptr_t)background_alpha | (uintptr_t)background_depth |
         (uintptr_t)background_normal | (uintptr_t)sky) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "an input image is not 4-B aligned");
    if (!mask || !original_rgb || !inpainted_rgb || !empty_opacity || !inpainted_depth || !inpainted_normal)
        return fail(SR_ERR_INVALID_ARGUMENT, "an output is NULL");
    if (threshold != threshold) return fail(SR_ERR_INVALID_ARGUMENT, "threshold is NaN");
    const UnveilConditions a{H, W, full_render, full_alpha, background_render, background_alpha, background_depth, background_normal, sky,
                             original_rgb, inpainted_rgb, empty_opacity, inpainted_depth, inpainted_normal};
    // two launches: the five images, the dilated instance mask
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(conditions_kernel, unveil_grid((size_t)H * (size_t)W), dim3(kUnveilThreads), 0, s, a);
    SR_HIP(launch_dilate(H, W, k, AlphaDiffSource{full_alpha, background_alpha, threshold}, mask, s));
    return SR_OK;
}

}  // extern "C"
