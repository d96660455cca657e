// image_loss.hip -- fused photometric loss of a training iteration (the reference's train.py:113-119 + utils/loss_utils.py:18-64):
//   x    = image (+ sky * (1 - alpha))                                   the composite is formed in the kernels, never written out
//   l1   = mean |x - y|,   ssim = mean ssim_map(x, y),   loss = (1 - lambda) * l1 + lambda * (1 - ssim)
//   ssim_map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   mu1 = G*x, s1 = G*x^2 - mu1^2, s12 = G*xy - mu1 mu2, ...
//   G = the 11x11 Gaussian window (sigma 1.5) with ZERO padding, not renormalised at the border; applied separably here.
// which the reference runs as five grouped 11x11 conv2d calls, ~10 element-wise kernels and the backward of all of them.
//
// Forward : per 32x16 pixel tile of one channel, x and y with a 5-pixel halo are staged in the LDS, a horizontal pass writes the five
//           row sums (x, y, x^2, y^2, xy) back to the LDS, a vertical pass finishes them.  Each pixel stores A, B, Cm (below) to the
//           caller's workspace; each workgroup walks its tiles in a fixed order and stores ONE partial sum of |x - y| and of ssim_map.
// Finalize: one workgroup adds the partials in a fixed order (in double) and writes loss, l1, ssim.  No float atomics anywhere.
// Backward: dL/dx = g (1-lambda)/N sign(x - y) - g lambda/N [ G*A + 2x (G*B) + y (G*Cm) ]
//           B = ds/d(s1), Cm = ds/d(s12), A = ds/d(mu1) - 2 mu1 B - mu2 Cm;  the same separable zero-padded window over three fields.
//           g is read from device memory.  With the composite: dL/dsky = (1 - alpha) dL/dx,  dL/dalpha = -sum_c sky_c dL/dx_c
//           (one workgroup walks the channels of its tile, so that sum needs no atomics either).
#include "abi.h"

namespace sr {

struct LossImages {       // a kernel parameter, by value
    int W, H, C;
    float lambda;
    const float* image;   // [C,H,W]
    const float* gt;      // [C,H,W]
    const float* sky;     // [C,H,W] or NULL
    const float* alpha;   // [1,H,W] or NULL (with sky)
};

constexpr int kLossTW = 32, kLossTH = 16, kLossR = 5;
constexpr int kLossSW = kLossTW + 2 * kLossR, kLossSH = kLossTH + 2 * kLossR;   // staged tile with its halo: 42 x 26
constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 4096;   // forward workgroups (= partial-sum slots of the workspace), whatever the frame size
constexpr float kLossC1 = 0.01f * 0.01f, kLossC2 = 0.03f * 0.03f;

// exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, rounded to float32 as the reference's window is
__device__ constexpr float kLossG[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                         0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

template <bool COMPOSITE>
__device__ __forceinline__ float loss_x_at(const LossImages& a, size_t HW, int c, size_t pix) {
    float x = a.image[c * HW + pix];
    if (COMPOSITE) x += a.sky[c * HW + pix] * (1.f - a.alpha[pix]);
    return x;
}

// sum of v over the workgroup, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float loss_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

template <bool COMPOSITE>
__global__ __launch_bounds__(kLossThreads) void image_loss_forward_kernel(LossImages a, int tiles_x, int tiles_y, int n_tiles,
                                                                          float* __restrict__ A, float* __restrict__ B,
                                                                          float* __restrict__ Cm, float* __restrict__ partials) {
    __shared__ float sx[kLossSH][kLossSW], sy[kLossSH][kLossSW];
    __shared__ float hs[5][kLossSH][kLossTW];
    __shared__ float red[kLossThreads];
    const int tid = threadIdx.x;
    const size_t HW = (size_t)a.W * a.H;
    float acc_l1 = 0.f, acc_ssim = 0.f;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int c = t / (tiles_x * tiles_y), rem = t - c * tiles_x * tiles_y;
        const int x0 = (rem % tiles_x) * kLossTW, y0 = (rem / tiles_x) * kLossTH;
        for (int i = tid; i < kLossSH * kLossSW; i += kLossThreads) {
            const int r = i / kLossSW, q = i - r * kLossSW;
            const int gx = x0 + q - kLossR, gy = y0 + r - kLossR;
            float xv = 0.f, yv = 0.f;
            if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
                const size_t pix = (size_t)gy * a.W + gx;
                xv = loss_x_at<COMPOSITE>(a, HW, c, pix);
                yv = a.gt[c * HW + pix];
            }
            sx[r][q] = xv;
            sy[r][q] = yv;
        }
        __syncthreads();
        for (int i = tid; i < kLossSH * kLossTW; i += kLossThreads) {
            const int r = i / kLossTW, q = i % kLossTW;
            float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float xv = sx[r][q + k], yv = sy[r][q + k], w = kLossG[k];
                m1 += w * xv; m2 += w * yv; xx += w * (xv * xv); yy += w * (yv * yv); xy += w * (xv * yv);
            }
            hs[0][r][q] = m1; hs[1][r][q] = m2; hs[2][r][q] = xx; hs[3][r][q] = yy; hs[4][r][q] = xy;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < kLossTH * kLossTW / kLossThreads; ++p) {
            const int r = tid / kLossTW + p * (kLossThreads / kLossTW), q = tid % kLossTW;
            const int gx = x0 + q, gy = y0 + r;
            if (gx < a.W && gy < a.H) {
                float mu1 = 0.f, mu2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const float w = kLossG[k];
                    mu1 += w * hs[0][r + k][q]; mu2 += w * hs[1][r + k][q]; xx += w * hs[2][r + k][q];
                    yy += w * hs[3][r + k][q]; xy += w * hs[4][r + k][q];
                }
                const float s1 = xx - mu1 * mu1, s2 = yy - mu2 * mu2, s12 = xy - mu1 * mu2;
                const float n1 = 2.f * mu1 * mu2 + kLossC1, n2 = 2.f * s12 + kLossC2;
                const float d1 = mu1 * mu1 + mu2 * mu2 + kLossC1, d2 = s1 + s2 + kLossC2;
                const float id1 = 1.f / d1, id2 = 1.f / d2;
                const float ssim = n1 * n2 * id1 * id2;
                const float b = -ssim * id2;                                            // ds/d(s1)
                const float cm = 2.f * n1 * id1 * id2;                                  // ds/d(s12)
                const float dmu1 = 2.f * (mu2 * n2 * id1 * id2 - mu1 * ssim * id1);     // ds/d(mu1) at fixed s1, s12
                const size_t o = c * HW + (size_t)gy * a.W + gx;
                A[o] = dmu1 - 2.f * mu1 * b - mu2 * cm;
                B[o] = b;
                Cm[o] = cm;
                acc_ssim += ssim;
                acc_l1 += fabsf(sx[r + kLossR][q + kLossR] - sy[r + kLossR][q + kLossR]);
            }
        }
        __syncthreads();   // the next tile restages sx / sy / hs
    }
    const float l1 = loss_block_sum(acc_l1, red);
    __syncthreads();
    const float ss = loss_block_sum(acc_ssim, red);
    if (tid == 0) { partials[2 * blockIdx.x] = l1; partials[2 * blockIdx.x + 1] = ss; }
}

// one workgroup: out = {loss, l1, ssim} from the n_blocks partial pairs, always added in the same order
__global__ __launch_bounds__(kLossThreads) void image_loss_finalize_kernel(const float* __restrict__ partials, int n_blocks, double inv_n,
                                                                           float lambda, float* __restrict__ out) {
    __shared__ double r1[kLossThreads], r2[kLossThreads];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += kLossThreads) { s1 += (double)partials[2 * i]; s2 += (double)partials[2 * i + 1]; }
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
#pragma unroll
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { r1[threadIdx.x] += r1[threadIdx.x + s]; r2[threadIdx.x] += r2[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(r1[0] * inv_n), ssim = (float)(r2[0] * inv_n);
        out[0] = (1.f - lambda) * l1 + lambda * (1.f - ssim);
        out[1] = l1;
        out[2] = ssim;
    }
}

// grid (tiles_x, tiles_y, COMPOSITE ? 1 : C): with the composite one workgroup walks all channels of its tile (dL/dalpha sums over them)
template <bool COMPOSITE>
__global__ __launch_bounds__(kLossThreads) void image_loss_backward_kernel(LossImages a, const float* __restrict__ A, const float* __restrict__ B,
                                                                           const float* __restrict__ Cm, const float* __restrict__ g_loss,
                                                                           float inv_n, float* __restrict__ g_image, float* __restrict__ g_sky,
                                                                           float* __restrict__ g_alpha) {
    __shared__ float sf[3][kLossSH][kLossSW];
    __shared__ float hs[3][kLossSH][kLossTW];
    constexpr int kPix = kLossTH * kLossTW / kLossThreads;
    const int tid = threadIdx.x;
    const size_t HW = (size_t)a.W * a.H;
    const int x0 = blockIdx.x * kLossTW, y0 = blockIdx.y * kLossTH;
    const int c_begin = COMPOSITE ? 0 : (int)blockIdx.z, c_end = COMPOSITE ? a.C : c_begin + 1;
    const float g = g_loss[0];
    const float k_l1 = g * (1.f - a.lambda) * inv_n, k_ssim = g * a.lambda * inv_n;
    float ga[kPix];
#pragma unroll
    for (int p = 0; p < kPix; ++p) ga[p] = 0.f;
    for (int c = c_begin; c < c_end; ++c) {
        for (int i = tid; i < kLossSH * kLossSW; i += kLossThreads) {
            const int r = i / kLossSW, q = i - r * kLossSW;
            const int gx = x0 + q - kLossR, gy = y0 + r - kLossR;
            float va = 0.f, vb = 0.f, vc = 0.f;
            if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
                const size_t o = c * HW + (size_t)gy * a.W + gx;
                va = A[o]; vb = B[o]; vc = Cm[o];
            }
            sf[0][r][q] = va; sf[1][r][q] = vb; sf[2][r][q] = vc;
        }
        __syncthreads();
        for (int i = tid; i < kLossSH * kLossTW; i += kLossThreads) {
            const int r = i / kLossTW, q = i % kLossTW;
            float ha = 0.f, hb = 0.f, hc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float w = kLossG[k];
                ha += w * sf[0][r][q + k]; hb += w * sf[1][r][q + k]; hc += w * sf[2][r][q + k];
            }
            hs[0][r][q] = ha; hs[1][r][q] = hb; hs[2][r][q] = hc;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            const int r = tid / kLossTW + p * (kLossThreads / kLossTW), q = tid % kLossTW;
            const int gx = x0 + q, gy = y0 + r;
            if (gx < a.W && gy < a.H) {
                float ca = 0.f, cb = 0.f, cc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const float w = kLossG[k];
                    ca += w * hs[0][r + k][q]; cb += w * hs[1][r + k][q]; cc += w * hs[2][r + k][q];
                }
                const size_t pix = (size_t)gy * a.W + gx;
                const float x = loss_x_at<COMPOSITE>(a, HW, c, pix), y = a.gt[c * HW + pix];
                const float d = x - y;
                const float sgn = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
                const float gxv = k_l1 * sgn - k_ssim * (ca + 2.f * x * cb + y * cc);
                g_image[c * HW + pix] = gxv;
                if (COMPOSITE) {
                    g_sky[c * HW + pix] = (1.f - a.alpha[pix]) * gxv;
                    ga[p] += a.sky[c * HW + pix] * gxv;
                }
            }
        }
        __syncthreads();   // the next channel restages sf / hs
    }
    if (COMPOSITE) {
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            const int r = tid / kLossTW + p * (kLossThreads / kLossTW), q = tid % kLossTW;
            const int gx = x0 + q, gy = y0 + r;
            if (gx < a.W && gy < a.H) g_alpha[(size_t)gy * a.W + gx] = -ga[p];
        }
    }
}

static inline int loss_tiles_x(int W) { return (W + kLossTW - 1) / kLossTW; }
static inline int loss_tiles_y(int H) { return (H + kLossTH - 1) / kLossTH; }

// the frame sizes the launches below can address: the tile count as an int, grid.y / grid.z within the launch limits
static bool image_loss_supported(int W, int H, int C) {
    const long long tiles = (long long)loss_tiles_x(W) * loss_tiles_y(H) * C;
    return tiles <= 0x7fffffffLL && loss_tiles_y(H) <= 65535 && C <= 65535;
}

// workspace: [kLossMaxBlocks][2] partial sums, then the planes A, B, Cm of [C,H,W] floats each
static size_t image_loss_partial_bytes() { return (size_t)kLossMaxBlocks * 2 * sizeof(float); }

static hipError_t launch_image_loss_forward(const LossImages& a, void* workspace, float* out3, hipStream_t s) {
    const size_t n = (size_t)a.W * a.H * a.C;
    float* partials = static_cast<float*>(workspace);
    float* A = partials + kLossMaxBlocks * 2;
    float *B = A + n, *Cm = B + n;
    const int tx = loss_tiles_x(a.W), ty = loss_tiles_y(a.H);
    const long long tiles = (long long)tx * ty * a.C;
    const int blocks = (int)(tiles < kLossMaxBlocks ? tiles : kLossMaxBlocks);
    if (a.sky)
        hipLaunchKernelGGL(image_loss_forward_kernel<true>, dim3(blocks), dim3(kLossThreads), 0, s, a, tx, ty, (int)tiles, A, B, Cm, partials);
    else
        hipLaunchKernelGGL(image_loss_forward_kernel<false>, dim3(blocks), dim3(kLossThreads), 0, s, a, tx, ty, (int)tiles, A, B, Cm, partials);
    hipLaunchKernelGGL(image_loss_finalize_kernel, dim3(1), dim3(kLossThreads), 0, s, partials, blocks, 1.0 / (double)n, a.lambda, out3);
    return hipGetLastError();
}

static hipError_t launch_image_loss_backward(const LossImages& a, const void* workspace, const float* g_loss, float* g_image, float* g_sky,
                                             float* g_alpha, hipStream_t s) {
    const size_t n = (size_t)a.W * a.H * a.C;
    const float* A = static_cast<const float*>(workspace) + kLossMaxBlocks * 2;
    const float *B = A + n, *Cm = B + n;
    const float inv_n = (float)(1.0 / (double)n);
    const int tx = loss_tiles_x(a.W), ty = loss_tiles_y(a.H);
    if (a.sky)
        hipLaunchKernelGGL(image_loss_backward_kernel<true>, dim3(tx, ty, 1), dim3(kLossThreads), 0, s, a, A, B, Cm, g_loss, inv_n, g_image,
                           g_sky, g_alpha);
    else
        hipLaunchKernelGGL(image_loss_backward_kernel<false>, dim3(tx, ty, a.C), dim3(kLossThreads), 0, s, a, A, B, Cm, g_loss, inv_n, g_image,
                           g_sky, g_alpha);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

extern "C" size_t sr_image_loss_workspace_bytes(int32_t W, int32_t H, int32_t C) {
    if (W <= 0 || H <= 0 || C <= 0) return 0;
    return image_loss_partial_bytes() + 3 * sizeof(float) * (size_t)W * (size_t)H * (size_t)C;
}

static int image_loss_args(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                           const float* alpha, const void* workspace, size_t workspace_bytes, LossImages* a) {
    if (W <= 0 || H <= 0 || C <= 0) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d with %d channels", W, H, C);
    if (!image || !gt || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "image / gt / workspace is NULL");
    if ((sky != nullptr) != (alpha != nullptr)) return fail(SR_ERR_INVALID_ARGUMENT, "sky and alpha go together: give both or neither");
    if (!image_loss_supported(W, H, C)) return fail(SR_ERR_UNSUPPORTED, "%dx%d with %d channels is beyond the launch limits", W, H, C);
    if (int rc = check_workspace_size(workspace, workspace_bytes, sr_image_loss_workspace_bytes(W, H, C))) return rc;
    *a = LossImages{W, H, C, lambda_dssim, image, gt, sky, alpha};
    return SR_OK;
}

extern "C" {

int sr_image_loss_forward(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                          const float* alpha, void* workspace, size_t workspace_bytes, float* out3, void* stream) {
    LossImages a;
    if (int rc = image_loss_args(W, H, C, lambda_dssim, image, gt, sky, alpha, workspace, workspace_bytes, &a)) return rc;
    if (!out3) return fail(SR_ERR_INVALID_ARGUMENT, "out3 is NULL");
    SR_HIP(launch_image_loss_forward(a, workspace, out3, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_image_loss_backward(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                           const float* alpha, const void* workspace, size_t workspace_bytes, const float* g_loss, float* g_image,
                           float* g_sky, float* g_alpha, void* stream) {
    LossImages a;
    if (int rc = image_loss_args(W, H, C, lambda_dssim, image, gt, sky, alpha, workspace, workspace_bytes, &a)) return rc;
    if (!g_loss || !g_image) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_image is NULL");
    if (sky && (!g_sky || !g_alpha)) return fail(SR_ERR_INVALID_ARGUMENT, "with sky and alpha, g_sky and g_alpha are required");
    SR_HIP(launch_image_loss_backward(a, workspace, g_loss, g_image, g_sky, g_alpha, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
