// resize.hip -- frame resizing with Pillow's 8-bit arithmetic, and nearest label maps (include/surfel_raster.h states the semantics):
//   [REF utils/camera_utils.py:22-73, utils/general_utils.py:21-27, inpainting_pipeline/3_reoptimization/1_optimization.py:140-199]
//     resize_pass_kernel<FLAGS>   one thread per output sample: one pass of the separable resize (axis 0 the columns, 1 the rows) through
//                                 the caller's integer tables, or (axis -1) no resampling at all; then the epilogue of the call -- the
//                                 byte in Pillow's [h,w,C] layout, 255 / 0 of it, or float32 v / 255 in [C,h,w]
//     nearest_kernel<T>           one thread per output element of a label map of 1-, 4- or 8-byte elements, copied as they are
//
// A resize is the horizontal pass, then the vertical pass on its uint8 result: two launches, the intermediate in global memory (1.8 MB
// for a 1920 x 1280 frame at a quarter of its size).  A block owns a tile of kResizeTileX samples of a row x kResizeTileY rows; for the
// byte layouts a row's samples are its w C bytes (a wave writes 64 consecutive bytes), for the float layout its w pixels of one channel
// (a wave writes 64 consecutive floats, the channel and the frame are grid.z).  In the vertical pass a wave reads 64 consecutive bytes
// (or every C-th of 64 C) per tap and the coefficient is the same for the whole wave; in the horizontal pass lane x starts at its own
// xmin(x) and the lanes of a wave walk neighbouring windows of one input row.
//
// The tables are the caller's (float64 on the host, rounded to integers there): bounds[o] = (first, count), coeffs[o * ksize + i].  They
// are device memory, which the host cannot check: the kernel clamps first into [0, in_size] and count into [0, min(ksize, in_size -
// first)] before it reads, so no table makes it read outside the frame.  The sum is a 32-bit two's-complement sum (held in a uint32_t:
// wrapping is defined), the shift arithmetic.  The division of the float epilogue is the IEEE one.  Integers apart from it: equal inputs
// give equal bits.
#include "abi.h"

namespace sr {

constexpr int kResizeTileX = 64;   // samples of a row a block covers: one wave a row
constexpr int kResizeTileY = 4;    // rows of a tile; the tile rows are grid.y: at most 4 * 65535 output rows
constexpr int kResizeBits = 22;    // Pillow's PRECISION_BITS

struct ResizePass {      // a kernel parameter, by value: device pointers
    int C;               // 1 or 3
    int axis;            // 0: resample the columns, 1: the rows, -1: neither
    int in_size;         // W (axis 0) or H (axis 1)
    int h, w;            // of the output
    int ksize;
    long long batch_stride, row_stride;   // of the input, in bytes; a pixel's C bytes are dense, a row's pixels too
    const uint8_t* in;
    const int32_t* bounds;
    const int32_t* coeffs;
};

template <uint32_t FLAGS>
__global__ __launch_bounds__(kResizeTileX * kResizeTileY) void resize_pass_kernel(ResizePass a, void* __restrict__ out) {
    constexpr bool kChw = (FLAGS & SR_RESIZE_F32_CHW) != 0;
    const int e = blockIdx.x * kResizeTileX + threadIdx.x;   // a row has at most 3 * 2^24 samples
    const int y = blockIdx.y * kResizeTileY + threadIdx.y;
    int n, c, x;
    if (kChw) {
        n = blockIdx.z / a.C;
        c = blockIdx.z - n * a.C;
        x = e;
    } else {
        n = blockIdx.z;
        x = e / a.C;
        c = e - x * a.C;
    }
    if (x >= a.w || y >= a.h) return;
    const uint8_t* img = a.in + (long long)n * a.batch_stride;
    int v;
    if (a.axis < 0) {
        v = img[(long long)y * a.row_stride + (long long)x * a.C + c];
    } else {
        const int o = a.axis == 0 ? x : y;
        const int first = min(max(a.bounds[2 * (long long)o], 0), a.in_size);
        const int count = min(min(a.bounds[2 * (long long)o + 1], a.ksize), a.in_size - first);
        const uint8_t* p = a.axis == 0 ? img + (long long)y * a.row_stride + (long long)first * a.C + c
                                       : img + (long long)first * a.row_stride + (long long)x * a.C + c;
        const long long step = a.axis == 0 ? (long long)a.C : a.row_stride;
        const int32_t* __restrict__ k = a.coeffs + (long long)o * a.ksize;
        uint32_t acc = 1u << (kResizeBits - 1);
        for (int i = 0; i < count; ++i) acc += (uint32_t)((int32_t)p[i * step] * k[i]);
        v = min(max((int32_t)acc >> kResizeBits, 0), 255);
    }
    if (kChw) {
        static_cast<float*>(out)[(((long long)n * a.C + c) * a.h + y) * a.w + x] = __fdiv_rn((float)v, 255.0f);
    } else {
        if (FLAGS & SR_RESIZE_BINARISE) v = v > 0 ? 255 : 0;
        static_cast<uint8_t*>(out)[(((long long)n * a.h + y) * a.w + x) * a.C + c] = (uint8_t)v;
    }
}

struct NearestMap {      // a kernel parameter, by value
    int H, W, h, w;
    float sy, sx;        // float32(H) / float32(h), float32(W) / float32(w)
    long long batch_stride, row_stride;   // of the input, in elements
};

template <class T>
__global__ __launch_bounds__(kResizeTileX * kResizeTileY) void nearest_kernel(NearestMap a, const T* __restrict__ in, T* __restrict__ out) {
    const int x = blockIdx.x * kResizeTileX + threadIdx.x;
    const int y = blockIdx.y * kResizeTileY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    // the product in float32, floor, then the clamp: torch's nearest rule (an output index is below 2^24: exact as a float)
    const int sy = min((int)floorf((float)y * a.sy), a.H - 1);
    const int sx = min((int)floorf((float)x * a.sx), a.W - 1);
    const long long n = blockIdx.z;
    out[(n * a.h + y) * a.w + x] = in[n * a.batch_stride + (long long)sy * a.row_stride + sx];
}

static dim3 resize_grid(long long row_samples, int rows, int planes) {
    return dim3((unsigned)((row_samples + kResizeTileX - 1) / kResizeTileX), (unsigned)((rows + kResizeTileY - 1) / kResizeTileY), (unsigned)planes);
}

static hipError_t launch_resize_pass(const ResizePass& a, int N, uint32_t flags, void* out, hipStream_t s) {
    const dim3 block(kResizeTileX, kResizeTileY);
    if (flags & SR_RESIZE_F32_CHW)
        hipLaunchKernelGGL(resize_pass_kernel<SR_RESIZE_F32_CHW>, resize_grid(a.w, a.h, N * a.C), block, 0, s, a, out);
    else if (flags & SR_RESIZE_BINARISE)
        hipLaunchKernelGGL(resize_pass_kernel<SR_RESIZE_BINARISE>, resize_grid((long long)a.w * a.C, a.h, N), block, 0, s, a, out);
    else
        hipLaunchKernelGGL(resize_pass_kernel<0u>, resize_grid((long long)a.w * a.C, a.h, N), block, 0, s, a, out);
    return hipGetLastError();
}

template <class T> static hipError_t launch_nearest(const NearestMap& a, int N, const void* in, void* out, hipStream_t s) {
    hipLaunchKernelGGL(nearest_kernel<T>, resize_grid(a.w, a.h, N), dim3(kResizeTileX, kResizeTileY), 0, s, a, static_cast<const T*>(in),
                       static_cast<T*>(out));
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// Both calls take raw addresses of memory the kernels read and write: an address the runtime does not know as device (or managed) memory
// -- a host tensor's -- is refused here, where the other ops leave that to their Python wrappers.
static int resize_device_pointer(const char* name, const void* p) {
    if (!p) return fail(SR_ERR_INVALID_ARGUMENT, "%s is NULL", name);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // an address it has never seen: the sticky error is cleared, the refusal is ours
        return fail(SR_ERR_INVALID_ARGUMENT, "%s is not device memory (a host address?)", name);
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
        return fail(SR_ERR_INVALID_ARGUMENT, "%s is not device memory (a host address?)", name);
    return SR_OK;
}

// what both calls ask of a frame or a map and of its output size; row_elems: the elements of a dense input row, planes: the launch's grid.z
static int resize_extents(int32_t N, int32_t H, int32_t W, int32_t h, int32_t w, long long row_elems, int64_t batch_stride, int64_t row_stride,
                          long long planes) {
    if (N < 1 || H < 1 || W < 1) return fail(SR_ERR_INVALID_ARGUMENT, "%d frames of %d x %d: N, H and W must be at least 1", N, H, W);
    if (h < 1 || w < 1) return fail(SR_ERR_INVALID_ARGUMENT, "an output of %d x %d: both sizes must be at least 1", w, h);
    if (H > (1 << 24) || W > (1 << 24) || h > (1 << 24) || w > (1 << 24)) return fail(SR_ERR_UNSUPPORTED, "a size above 2^24");
    if (h > kResizeTileY * 65535) return fail(SR_ERR_UNSUPPORTED, "an output of %d rows: at most %d", h, kResizeTileY * 65535);
    if (planes > 65535) return fail(SR_ERR_UNSUPPORTED, "%lld frames (x channels of a float output): at most 65535 a call", planes);
    if (row_stride < row_elems) return fail(SR_ERR_INVALID_ARGUMENT, "in_row_stride %lld < the %lld of a dense row", (long long)row_stride, row_elems);
    if (batch_stride < 0) return fail(SR_ERR_INVALID_ARGUMENT, "in_batch_stride %lld is negative", (long long)batch_stride);
    return SR_OK;
}

extern "C" {

int sr_resize_u8_pass(int32_t N, int32_t H, int32_t W, int32_t C, const uint8_t* in, int64_t in_batch_stride, int64_t in_row_stride, int32_t axis,
                      int32_t out_size, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, uint32_t flags, void* out, void* stream) {
    if (C != 1 && C != 3) return fail(SR_ERR_UNSUPPORTED, "C = %d channels: 1 or 3 (an alpha channel is resized through premultiplied alpha, which is not built)", C);
    if (axis < -1 || axis > 1) return fail(SR_ERR_INVALID_ARGUMENT, "axis = %d: 0 (columns), 1 (rows) or -1 (no resampling)", axis);
    if (flags & ~(uint32_t)(SR_RESIZE_BINARISE | SR_RESIZE_F32_CHW)) return fail(SR_ERR_INVALID_ARGUMENT, "flags 0x%x: unknown bits", flags);
    if ((flags & SR_RESIZE_BINARISE) && (flags & SR_RESIZE_F32_CHW))
        return fail(SR_ERR_INVALID_ARGUMENT, "SR_RESIZE_BINARISE with SR_RESIZE_F32_CHW: the 255 / 0 mask is a uint8 output");
    if (axis >= 0 && out_size < 1) return fail(SR_ERR_INVALID_ARGUMENT, "out_size = %d: must be at least 1", out_size);
    const int32_t h = axis == 1 ? out_size : H, w = axis == 0 ? out_size : W;
    const bool chw = (flags & SR_RESIZE_F32_CHW) != 0;
    if (int rc = resize_extents(N, H, W, h, w, (long long)W * C, in_batch_stride, in_row_stride, (long long)N * (chw ? C : 1))) return rc;
    if (axis >= 0 && ksize < 1) return fail(SR_ERR_INVALID_ARGUMENT, "ksize = %d: must be at least 1", ksize);
    if (int rc = resize_device_pointer("in", in)) return rc;
    if (int rc = resize_device_pointer("out", out)) return rc;
    if (chw && ((uintptr_t)out & 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "out is not 4-B aligned");
    if (axis >= 0) {
        if (int rc = resize_device_pointer("bounds", bounds)) return rc;
        if (int rc = resize_device_pointer("coeffs", coeffs)) return rc;
        if (((uintptr_t)bounds | (uintptr_t)coeffs) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "bounds / coeffs is not 4-B aligned");
    }
    if ((const void*)in == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the input: a sample reads its neighbours");
    const ResizePass a{C, axis, axis == 0 ? W : H, h, w, axis >= 0 ? ksize : 0, in_batch_stride, in_row_stride, in, bounds, coeffs};
    SR_HIP(launch_resize_pass(a, N, flags, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_resize_nearest(int32_t N, int32_t H, int32_t W, int32_t elem_bytes, const void* in, int64_t in_batch_stride, int64_t in_row_stride, int32_t h,
                      int32_t w, void* out, void* stream) {
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) return fail(SR_ERR_UNSUPPORTED, "elem_bytes = %d: 1, 4 or 8", elem_bytes);
    if (int rc = resize_extents(N, H, W, h, w, W, in_batch_stride, in_row_stride, N)) return rc;
    if (int rc = resize_device_pointer("in", in)) return rc;
    if (int rc = resize_device_pointer("out", out)) return rc;
    if (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(elem_bytes - 1)) return fail(SR_ERR_INVALID_ARGUMENT, "in / out is not aligned to its element size");
    if (in == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the input");
    const NearestMap a{H, W, h, w, (float)H / (float)h, (float)W / (float)w, in_batch_stride, in_row_stride};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 1) SR_HIP(launch_nearest<uint8_t>(a, N, in, out, s));
    else if (elem_bytes == 4) SR_HIP(launch_nearest<uint32_t>(a, N, in, out, s));
    else SR_HIP(launch_nearest<unsigned long long>(a, N, in, out, s));
    return SR_OK;
}

}  // extern "C"
