// sky.hip -- the per-pixel part of the sky model (the reference's scene/env_map.py SkyModel.render_with_camera), forward and backward.
// Every pixel of a frame hands the model the SAME position, so of the MLP's 111 inputs only the 16 SH channels of the ray direction
// differ per pixel; the other 95 fold into one 64-vector per frame, c = W0[:, 16:] feat + b0, which the caller forms.  Per pixel:
//   dir = R ((i - cx) / fx, -(j - cy) / fy, -1)   (not normalised),   sh = the 16 degree-4 polynomials of torch-ngp's shencoder,
//   h1 = relu(W0sh sh + c),  h2 = relu(W1 h1 + b1),  h3 = relu(W2 h2 + b2),  out = sigmoid(W3 h3 + b3)            all float32.
// The 9603 weights {W0sh[64,16] c[64] W1[64,64] b1[64] W2[64,64] b2[64] W3[3,64] b3[3]} sit in the LDS in that order (SkyOff); every
// lane of a wave reads the same weight at the same time (identical addresses broadcast: no bank conflict).
//   forward    one thread owns one pixel; its 64 activations are registers (every loop is unrolled, no array is indexed at run time).
//   backward   a persistent grid: a workgroup takes 256 pixels at a time, each thread recomputes its pixel's activations and forms its
//              deltas in registers; a weight gradient sum_p delta_i(p) h_k(p) is taken 64 pixels (one wave) at a time through two LDS
//              panels, thread t owning a fixed set of (i, k) entries: a float32 fma chain over the panel's pixels in order, then added to
//              the workgroup's float64 sums in the LDS.  Each workgroup stores its 9603 sums once; sky_finalize_kernel adds the
//              workgroups' sets in index order and rounds once.  No atomics: the order of every addition follows from (W, H, the
//              workgroup count) alone, so two calls on equal inputs give equal bits.
// relu keeps a NaN (x < 0 ? 0 : x) and its derivative is torch's threshold_backward (h <= 0 ? 0 : g).
#include "abi.h"

namespace sr {

constexpr int kSkyParams = 64 * 16 + 64 + 2 * (64 * 64 + 64) + 3 * 64 + 3;   // 9603: {W0sh c W1 b1 W2 b2 W3 b3}
constexpr int kSkyParamsPadded = kSkyParams + 1;
constexpr int kSkyDefaultForwardGroups = 1024;    // workgroups of 256 pixels where max_workgroups == 0: a few per CU
constexpr int kSkyDefaultBackwardGroups = 256;    // one per CU: its sums, weights and panels take most of a CU's LDS
constexpr int kSkyMaxGroups = 1 << 16;
struct SkyWeights {        // a kernel parameter, by value: device pointers
    const float *w0sh, *c, *w1, *b1, *w2, *b2, *w3, *b3;
};

namespace {

constexpr int kSkyThreads = 256;
constexpr int kSkyWaves = kSkyThreads / 64;
constexpr int kHid = 64, kShN = 16;
constexpr int kPanelStride = 65;                         // floats per panel row: row r, pixel p in bank (r + p) mod 32
constexpr int kPanelFloats = kHid * kPanelStride;
constexpr size_t kSkyBackwardLds = (size_t)(kSkyParamsPadded + 2 * kPanelFloats) * sizeof(float) + kSkyParams * sizeof(double);
static_assert((kSkyParamsPadded + 2 * kPanelFloats) % 2 == 0, "the float64 sums behind the float32 regions are 8-byte aligned");
static_assert(kSkyBackwardLds <= 160 * 1024, "the backward's sums, weights and panels fit the 160 KiB of a CU");

struct SkyOff {   // float offsets of the parameter set, in the LDS and in every gradient set (16-byte aligned where rows are read whole)
    static constexpr int W0 = 0, C = 1024, W1 = 1088, B1 = 5184, W2 = 5248, B2 = 9344, W3 = 9408, B3 = 9600;
};
static_assert(SkyOff::B3 + 3 == kSkyParams, "the parameter set is 9603 floats");

__device__ __forceinline__ void sky_load_weights(float* w, const SkyWeights& p) {
    const int t = threadIdx.x;
    for (int e = t; e < kHid * kShN; e += kSkyThreads) w[SkyOff::W0 + e] = p.w0sh[e];
    for (int e = t; e < kHid * kHid; e += kSkyThreads) { w[SkyOff::W1 + e] = p.w1[e]; w[SkyOff::W2 + e] = p.w2[e]; }
    if (t < kHid) { w[SkyOff::C + t] = p.c[t]; w[SkyOff::B1 + t] = p.b1[t]; w[SkyOff::B2 + t] = p.b2[t]; }
    if (t < 3 * kHid) w[SkyOff::W3 + t] = p.w3[t];
    if (t < 3) w[SkyOff::B3 + t] = p.b3[t];
}

// torch-ngp's shencoder, degree 4, on the UNNORMALISED direction (not the rasterizer's basis of sh.h: other signs, other argument)
__device__ __forceinline__ void sky_sh(float x, float y, float z, float (&sh)[kShN]) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    sh[0] = 0.28209479177387814f;
    sh[1] = -0.48860251190291987f * y;
    sh[2] = 0.48860251190291987f * z;
    sh[3] = -0.48860251190291987f * x;
    sh[4] = 1.0925484305920792f * xy;
    sh[5] = -1.0925484305920792f * yz;
    sh[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    sh[7] = -1.0925484305920792f * xz;
    sh[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    sh[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    sh[10] = 2.8906114426405538f * xy * z;
    sh[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    sh[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    sh[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    sh[14] = 1.4453057213202769f * z * (x2 - y2);
    sh[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}

// cam = {fx, fy, cx, cy, R[9] row-major}: the reference's get_rays for pixel column i, row j, then the encoding
__device__ __forceinline__ void sky_pixel_sh(const float* __restrict__ cam, int W, size_t pix, float (&sh)[kShN]) {
    const float i = (float)(int)(pix % (size_t)W), j = (float)(int)(pix / (size_t)W);
    const float dx = (i - cam[2]) / cam[0], dy = -(j - cam[3]) / cam[1], dz = -1.0f;
    const float x = dx * cam[4] + dy * cam[5] + dz * cam[6];
    const float y = dx * cam[7] + dy * cam[8] + dz * cam[9];
    const float z = dx * cam[10] + dy * cam[11] + dz * cam[12];
    sky_sh(x, y, z, sh);
}

__device__ __forceinline__ float sky_relu(float x) { return x < 0.0f ? 0.0f : x; }

// The weights are read from the LDS where they are used, every time: without this fence the compiler keeps thousands of them (they
// do not change inside the pixel loop) in registers and spills.  Between two fences at most 32 weights are in flight.
__device__ __forceinline__ void sky_reread_weights() { asm volatile("" ::: "memory"); }
// The same fence, which also wants the running sums of the group before it: their fmas cannot drift away from the reads they consume.
__device__ __forceinline__ void sky_reread_weights(float (&a)[8]) {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) : : "memory");
}
__device__ __forceinline__ void sky_reread_weights(float (&a)[16]) {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]),
                 "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]) : : "memory");
}
// A sum that a relu mask then keeps or drops is computed HERE, for every lane: left alone, the compiler moves its fma chain behind a
// branch on the mask, far from the weight reads the fences hold in place, and spills those weights in between.
__device__ __forceinline__ float sky_computed_here(float v) { asm volatile("" : "+v"(v)); return v; }

// out = relu(W in + b), W [64, IN] row-major at w + w_off, b at w + b_off: eight outputs at a time, each a fma chain over k in order
template <int IN>
__device__ __forceinline__ void sky_layer(const float* w, int w_off, int b_off, const float (&in)[IN], float (&out)[kHid]) {
#pragma unroll
    for (int j0 = 0; j0 < kHid; j0 += 8) {
        float acc[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) acc[jj] = w[b_off + j0 + jj];
#pragma unroll
        for (int k0 = 0; k0 < IN; k0 += 4) {
            sky_reread_weights(acc);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[jj] = fmaf(w[w_off + (j0 + jj) * IN + k0 + kk], in[k0 + kk], acc[jj]);
            }
        }
        sky_reread_weights(acc);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) out[j0 + jj] = sky_relu(acc[jj]);
    }
}

__device__ __forceinline__ void sky_output(const float* w, const float (&h3)[kHid], float (&o)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sky_reread_weights();
        float acc = w[SkyOff::B3 + c];
#pragma unroll
        for (int k = 0; k < kHid; ++k) acc = fmaf(w[SkyOff::W3 + c * kHid + k], h3[k], acc);
        o[c] = 1.0f / (1.0f + expf(-acc));
    }
}

// h <- (h <= 0 ? 0 : sum_j W[j][k] d[j]): the delta of the layer below, written over that layer's activations, 16 outputs at a time
__device__ __forceinline__ void sky_delta_below(const float* w, int w_off, const float (&d)[kHid], float (&h)[kHid]) {
#pragma unroll
    for (int k0 = 0; k0 < kHid; k0 += 16) {
        float acc[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc[kk] = 0.0f;
#pragma unroll
        for (int j = 0; j < kHid; ++j) {
            if (j % 2 == 0) sky_reread_weights(acc);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) acc[kk] = fmaf(w[w_off + j * kHid + k0 + kk], d[j], acc[kk]);
        }
        sky_reread_weights(acc);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) h[k0 + kk] = h[k0 + kk] <= 0.0f ? 0.0f : acc[kk];
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSkyThreads) void sky_forward_kernel(int W, size_t N, const float* __restrict__ cam, SkyWeights p,
                                                                  float* __restrict__ out) {
    __shared__ __align__(16) float w[kSkyParamsPadded];
    sky_load_weights(w, p);
    __syncthreads();
    for (size_t pix = (size_t)blockIdx.x * kSkyThreads + threadIdx.x; pix < N; pix += (size_t)gridDim.x * kSkyThreads) {
        float sh[kShN], a[kHid], b[kHid], o[3];
        sky_pixel_sh(cam, W, pix, sh);
        sky_layer<kShN>(w, SkyOff::W0, SkyOff::C, sh, a);
        sky_layer<kHid>(w, SkyOff::W1, SkyOff::B1, a, b);
        sky_layer<kHid>(w, SkyOff::W2, SkyOff::B2, b, a);
        sky_output(w, a, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(size_t)c * N + pix] = o[c];
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// One wave at a time hands its 64 pixels' rows to the two panels; then every thread adds its entries.  NA x NB entries per thread:
// rows ra0 + a * sa of the left panel times rows rb0 + b * sb of the right one -> sums[g_off + row_a * ncols + row_b].
template <int NA, int NB>
__device__ __forceinline__ void sky_add_products(const float* pa, const float* pb, int ra0, int sa, int rb0, int sb, double* sums, int g_off,
                                                 int ncols) {
    float acc[NA][NB];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = 0.0f;
#pragma unroll 4
    for (int q = 0; q < 64; ++q) {
        float va[NA], vb[NB];
#pragma unroll
        for (int a = 0; a < NA; ++a) va[a] = pa[(ra0 + a * sa) * kPanelStride + q];
#pragma unroll
        for (int b = 0; b < NB; ++b) vb[b] = pb[(rb0 + b * sb) * kPanelStride + q];
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[a][b] = fmaf(va[a], vb[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) sums[g_off + (ra0 + a * sa) * ncols + rb0 + b * sb] += (double)acc[a][b];
}

// sums[g_off + row] += the sum of the left panel's row over its 64 pixels, for the threads t < rows
__device__ __forceinline__ void sky_add_rows(const float* pa, int rows, double* sums, int g_off) {
    const int t = threadIdx.x;
    if (t >= rows) return;
    float acc = 0.0f;
#pragma unroll 4
    for (int q = 0; q < 64; ++q) acc += pa[t * kPanelStride + q];
    sums[g_off + t] += (double)acc;
}

enum class SkyGrad { kW3, kHidden, kW0 };

// the gradient of one layer: left rows = the deltas d[0..ND), right rows = the inputs x[0..NX); `bias_off`: where sum_p d goes
template <SkyGrad WHICH, int ND, int NX>
__device__ __forceinline__ void sky_layer_gradient(float* pa, float* pb, const float (&d)[ND], const float (&x)[NX], double* sums, int w_off,
                                                   int bias_off) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
#pragma unroll 1
    for (int turn = 0; turn < kSkyWaves; ++turn) {
        __syncthreads();   // the panels' last readers are done
        if (wave == turn) {
#pragma unroll
            for (int i = 0; i < ND; ++i) pa[i * kPanelStride + lane] = d[i];
#pragma unroll
            for (int k = 0; k < NX; ++k) pb[k * kPanelStride + lane] = x[k];
        }
        __syncthreads();
        if (WHICH == SkyGrad::kHidden) sky_add_products<4, 4>(pa, pb, (t >> 4) * 4, 1, t & 15, 16, sums, w_off, kHid);
        if (WHICH == SkyGrad::kW0) sky_add_products<1, 4>(pa, pb, t >> 2, 1, t & 3, 4, sums, w_off, kShN);
        if (WHICH == SkyGrad::kW3 && t < 3 * kHid) sky_add_products<1, 1>(pa, pb, t >> 6, 1, t & 63, 1, sums, w_off, kHid);
        sky_add_rows(pa, ND, sums, bias_off);
    }
}

__global__ __launch_bounds__(kSkyThreads) void sky_backward_kernel(int W, size_t N, const float* __restrict__ cam, SkyWeights p,
                                                                   const float* __restrict__ g_out, double* __restrict__ partials) {
    extern __shared__ __align__(16) unsigned char lds[];
    // the weights first: every read of one is an immediate offset below the 64 KiB a DS instruction can encode
    float* w = reinterpret_cast<float*>(lds);
    float* pa = w + kSkyParamsPadded;
    float* pb = pa + kPanelFloats;
    double* sums = reinterpret_cast<double*>(pb + kPanelFloats);      // [kSkyParams]: entry e is touched by one thread only
    const int t = threadIdx.x;
    for (int e = t; e < kSkyParams; e += kSkyThreads) sums[e] = 0.0;
    sky_load_weights(w, p);
    __syncthreads();

    for (size_t base = (size_t)blockIdx.x * kSkyThreads; base < N; base += (size_t)gridDim.x * kSkyThreads) {   // uniform per workgroup
        const bool valid = base + t < N;
        const size_t pix = valid ? base + t : 0;   // a thread past the end computes pixel 0 with a zero upstream gradient
        float sh[kShN], ha[kHid], hb[kHid], o[3], d_out[3];
        sky_pixel_sh(cam, W, pix, sh);
        sky_layer<kShN>(w, SkyOff::W0, SkyOff::C, sh, ha);            // h1
        sky_layer<kHid>(w, SkyOff::W1, SkyOff::B1, ha, hb);           // h2
        sky_layer<kHid>(w, SkyOff::W2, SkyOff::B2, hb, ha);           // h3 (h1 is recomputed below)
        sky_output(w, ha, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) d_out[c] = valid ? g_out[(size_t)c * N + pix] * (o[c] * (1.0f - o[c])) : 0.0f;
        if (!valid) {
#pragma unroll
            for (int k = 0; k < kHid; ++k) { ha[k] = 0.0f; hb[k] = 0.0f; }
#pragma unroll
            for (int k = 0; k < kShN; ++k) sh[k] = 0.0f;
        }
        sky_layer_gradient<SkyGrad::kW3, 3, kHid>(pa, pb, d_out, ha, sums, SkyOff::W3, SkyOff::B3);
#pragma unroll
        for (int k = 0; k < kHid; ++k) {                              // ha <- delta3
            if (k % 8 == 0) sky_reread_weights();
            const float s = fmaf(w[SkyOff::W3 + 2 * kHid + k], d_out[2], fmaf(w[SkyOff::W3 + kHid + k], d_out[1], w[SkyOff::W3 + k] * d_out[0]));
            ha[k] = ha[k] <= 0.0f ? 0.0f : sky_computed_here(s);
        }
        sky_layer_gradient<SkyGrad::kHidden, kHid, kHid>(pa, pb, ha, hb, sums, SkyOff::W2, SkyOff::B2);
        sky_delta_below(w, SkyOff::W2, ha, hb);                       // hb <- delta2
        sky_layer<kShN>(w, SkyOff::W0, SkyOff::C, sh, ha);            // ha <- h1 again
        if (!valid) {
#pragma unroll
            for (int k = 0; k < kHid; ++k) ha[k] = 0.0f;
        }
        sky_layer_gradient<SkyGrad::kHidden, kHid, kHid>(pa, pb, hb, ha, sums, SkyOff::W1, SkyOff::B1);
        sky_delta_below(w, SkyOff::W1, hb, ha);                       // ha <- delta1
        sky_layer_gradient<SkyGrad::kW0, kHid, kShN>(pa, pb, ha, sh, sums, SkyOff::W0, SkyOff::C);
    }
    __syncthreads();
    double* mine = partials + (size_t)blockIdx.x * kSkyParams;
    for (int e = t; e < kSkyParams; e += kSkyThreads) mine[e] = sums[e];
}

struct SkyGradOut {
    float* p[8];   // g_w0sh, g_c, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3; nullptr = not wanted
};

// entry e of the parameter set: the workgroups' sums in index order, rounded once, into the tensor that holds it
__global__ __launch_bounds__(kSkyThreads) void sky_finalize_kernel(const double* __restrict__ partials, int n_groups, SkyGradOut out) {
    const int e = blockIdx.x * kSkyThreads + threadIdx.x;
    if (e >= kSkyParams) return;
    double s = 0.0;
    for (int g = 0; g < n_groups; ++g) s += partials[(size_t)g * kSkyParams + e];
    const int starts[9] = {SkyOff::W0, SkyOff::C, SkyOff::W1, SkyOff::B1, SkyOff::W2, SkyOff::B2, SkyOff::W3, SkyOff::B3, kSkyParams};
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (e >= starts[k] && e < starts[k + 1] && out.p[k]) out.p[k][e - starts[k]] = (float)s;
}

int sky_groups(size_t N, int max_workgroups, int fallback) {
    const size_t need = (N + kSkyThreads - 1) / kSkyThreads;
    const size_t cap = (size_t)(max_workgroups > 0 ? max_workgroups : fallback);
    return (int)(need < cap ? need : cap);
}

int sky_backward_groups(int max_workgroups) { return max_workgroups > 0 ? max_workgroups : kSkyDefaultBackwardGroups; }
// the float64 parameter-gradient set of every workgroup of the backward
size_t sky_workspace_bytes(int max_workgroups) { return align_up((size_t)sky_backward_groups(max_workgroups) * kSkyParams * sizeof(double), 256); }

// grads: g_w0sh, g_c, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3; a NULL pointer is skipped
hipError_t launch_sky_backward(int W, int H, const float* cam, const SkyWeights& p, const float* g_out, int max_workgroups, void* workspace,
                               float* const (&grads)[8], hipStream_t s) {
    const size_t N = (size_t)W * (size_t)H;
    // more than the 64 KiB a kernel gets unasked; per device, so on every call (a host-side setting: nothing is enqueued)
    const hipError_t lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(sky_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)kSkyBackwardLds);
    if (lds_ok != hipSuccess) return lds_ok;
    double* partials = static_cast<double*>(workspace);
    const int groups = sky_groups(N, max_workgroups, kSkyDefaultBackwardGroups);
    hipLaunchKernelGGL(sky_backward_kernel, dim3(groups), dim3(kSkyThreads), kSkyBackwardLds, s, W, N, cam, p, g_out, partials);
    SkyGradOut out;
    for (int k = 0; k < 8; ++k) out.p[k] = grads[k];
    hipLaunchKernelGGL(sky_finalize_kernel, dim3((kSkyParams + kSkyThreads - 1) / kSkyThreads), dim3(kSkyThreads), 0, s, partials, groups, out);
    return hipGetLastError();
}

}  // namespace

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

static int sky_args(const char* what, int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1,
                    const float* w2, const float* b2, const float* w3, const float* b3, int32_t max_workgroups, SkyWeights* p) {
    if (W < 0 || H < 0) return fail(SR_ERR_INVALID_ARGUMENT, "%s: bad image size %dx%d", what, W, H);
    if (max_workgroups < 0 || max_workgroups > kSkyMaxGroups)
        return fail(SR_ERR_INVALID_ARGUMENT, "%s: max_workgroups %d not in 0..%d", what, max_workgroups, kSkyMaxGroups);
    if ((int64_t)W * (int64_t)H > 0x7fffffffll) return fail(SR_ERR_UNSUPPORTED, "%s: %dx%d is 2^31 pixels or more", what, W, H);
    if (!cam || !w0sh || !c || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return fail(SR_ERR_INVALID_ARGUMENT, "%s: cam or a weight pointer is NULL", what);
    *p = SkyWeights{w0sh, c, w1, b1, w2, b2, w3, b3};
    return SR_OK;
}

extern "C" {

size_t sr_sky_workspace_bytes(int32_t max_workgroups) { return max_workgroups >= 0 ? sky_workspace_bytes(max_workgroups) : 0; }

int sr_sky_forward(int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, int32_t max_workgroups, float* out, void* stream) {
    SkyWeights p;
    if (int rc = sky_args("sr_sky_forward", W, H, cam, w0sh, c, w1, b1, w2, b2, w3, b3, max_workgroups, &p)) return rc;
    if (W == 0 || H == 0) return SR_OK;
    if (!out) return fail(SR_ERR_INVALID_ARGUMENT, "sr_sky_forward: out is NULL");
    const size_t N = (size_t)W * (size_t)H;
    hipLaunchKernelGGL(sky_forward_kernel, dim3(sky_groups(N, max_workgroups, kSkyDefaultForwardGroups)), dim3(kSkyThreads), 0,
                       static_cast<hipStream_t>(stream), W, N, cam, p, out);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

int sr_sky_backward(int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* w3, const float* b3, const float* g_out, int32_t max_workgroups, void* workspace,
                    size_t workspace_bytes, float* g_w0sh, float* g_c, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3,
                    void* stream) {
    SkyWeights p;
    if (int rc = sky_args("sr_sky_backward", W, H, cam, w0sh, c, w1, b1, w2, b2, w3, b3, max_workgroups, &p)) return rc;
    if (W == 0 || H == 0) return SR_OK;
    if (!g_out) return fail(SR_ERR_INVALID_ARGUMENT, "sr_sky_backward: g_out is NULL");
    float* const grads[8] = {g_w0sh, g_c, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
    bool any = false;
    for (float* g : grads) any = any || g != nullptr;
    if (!any) return SR_OK;
    if (int rc = check_workspace_size(workspace, workspace_bytes, sky_workspace_bytes(max_workgroups), "sr_sky_backward")) return rc;
    SR_HIP(launch_sky_backward(W, H, cam, p, g_out, max_workgroups, workspace, grads, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
