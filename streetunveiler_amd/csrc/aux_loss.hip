// aux_loss.hip -- the losses of a training iteration beside the image loss (the reference's train.py:87-88 and :124-143; the unveiling
// stage's 1_optimization.py:249-256), each as one forward kernel + the finalize workgroup of reduce.h and one backward kernel:
//   semantic cross-entropy   loss = (1/N) sum_pix -sum_c w_c t_c (x_c - lse(x)),   lse(x) = m + log sum_c exp(x_c - m),  m = max_c x_c
//                            == F.cross_entropy(x[None], t[None], weight=w) with probability targets (torch divides by N, not by sum w).
//                            t is a [C,H,W] float image, or -- the hot path -- an [H,W] label map whose one-hot image is never built:
//                            term = -w[l] (x[l] - lse(x)); a label outside 0..C-1 has an all-zero row: 0 * lse(x), it counts in N.
//                            d/dx_c = (g/N) (softmax_c S - w_c t_c),  S = sum_k w_k t_k  (labels: w[l] or 0); the softmax is recomputed.
//   surface regularisers     normal = mean(1 - sum_c rn_c sn_c),  dist = mean(rend_dist),  out = {ln normal + ld dist, ln normal, ld dist}
//                            d/drn = -(g ln/N) sn,  d/dsn = -(g ln/N) rn,  d/ddist = g ld/N
//   opacity shrink           mean(sigmoid(raw)) with d/draw = (g/P) s (1 - s), or mean(o) with d/do = g/P of activated opacities
// One thread per pixel / Gaussian, planar coalesced loads.  These kernels wait for HBM, so the arithmetic is done in float64: every term
// and every gradient element is the float64 expression of its float32 inputs, rounded to float32 ONCE, at the store; the sums stay
// float64 up to the store of the loss.  No atomics, no host read-back; g is read from device memory, so a captured graph replays with
// whatever the upstream scalar then holds.
#include "abi.h"
#include "reduce.h"

namespace sr {

constexpr int kCeMaxClasses = 8;
static_assert(SR_CE_MAX_CLASSES == kCeMaxClasses, "the header's class limit is the kernels'");
enum class CeTarget { kProbabilities = 0, kLabelsU8 = 1, kLabelsI32 = 4, kLabelsI64 = 8 };   // the labels' values are their widths in bytes
struct CeArgs {            // a kernel parameter, by value: the class weights travel in the launch
    int C;
    size_t N;              // H * W
    float w[kCeMaxClasses];
    const float* x;        // [C,H,W] logits
    const void* target;    // [H,W] labels or [C,H,W] float probabilities
};
struct SurfaceRegArgs {    // a kernel parameter, by value
    size_t N;
    double lambda_normal, lambda_dist;
    const float* rend_normal;   // [3,H,W]
    const float* surf_normal;   // [3,H,W]
    const float* rend_dist;     // [1,H,W]
};

constexpr int kAuxThreads = kReduceThreads;   // one pixel / Gaussian per thread; one partial (pair) per workgroup

static inline size_t aux_blocks(size_t n) { return (n + kAuxThreads - 1) / kAuxThreads; }

static bool aux_loss_supported(size_t n) { return aux_blocks(n) <= 0x7fffffffull; }              // the element counts the launches can address
static size_t aux_loss_workspace_bytes(size_t n) { return aux_blocks(n) * 2 * sizeof(double); }   // per-block partial sums of n pixels / Gaussians

// ---- finalize: one workgroup; K == 1: out[0] = w0 * sum0 / n;  K == 2: out = {a + b, a, b},  a = w0 * sum0 / n,  b = w1 * sum1 / n ---------
template <int K>
__global__ __launch_bounds__(kReduceThreads) void aux_finalize_kernel(const double* __restrict__ partials, int n_blocks, double n, double w0,
                                                                     double w1, float* __restrict__ out) {
    __shared__ double red[kReduceThreads];
    double sums[K];
    finalize_sums<K>(partials, n_blocks, red, sums);
    if (threadIdx.x == 0) {
        const double a = w0 * (sums[0] / n);
        if (K == 1) {
            out[0] = (float)a;
        } else {
            const double b = w1 * (sums[K - 1] / n);
            out[0] = (float)(a + b);
            out[1] = (float)a;
            out[2] = (float)b;
        }
    }
}

// ---- semantic cross-entropy ----------------------------------------------------------------------------------------------------------
template <CeTarget FORM>
__device__ __forceinline__ long long ce_label(const void* target, size_t pix) {
    if (FORM == CeTarget::kLabelsU8) return static_cast<const uint8_t*>(target)[pix];
    if (FORM == CeTarget::kLabelsI32) return static_cast<const int32_t*>(target)[pix];
    return static_cast<const int64_t*>(target)[pix];
}

struct CePixel {
    double d[kCeMaxClasses];    // x_c - m
    double e[kCeMaxClasses];    // exp(x_c - m)
    double wt[kCeMaxClasses];   // w_c t_c
    double s;                   // sum_c e_c
    double S;                   // sum_c w_c t_c
    double dl;                  // labels: d of the label's class (0 outside the range)
};

// Every loop runs over kCeMaxClasses with its body under `c < C`, fully unrolled: no array is indexed with a run-time value (the label
// picks its class by comparison), so everything stays in registers.
template <CeTarget FORM>
__device__ __forceinline__ void ce_pixel(const CeArgs& a, size_t pix, CePixel& p) {
    float x[kCeMaxClasses];
#pragma unroll
    for (int c = 0; c < kCeMaxClasses; ++c) x[c] = c < a.C ? a.x[(size_t)c * a.N + pix] : 0.f;
    float m = x[0];
#pragma unroll
    for (int c = 1; c < kCeMaxClasses; ++c)
        if (c < a.C) m = fmaxf(m, x[c]);   // drops a NaN: the sum of the exponentials below carries it
    p.s = 0.0;
#pragma unroll
    for (int c = 0; c < kCeMaxClasses; ++c) {
        p.d[c] = (double)x[c] - (double)m;
        p.e[c] = c < a.C ? exp(p.d[c]) : 0.0;
        p.s += p.e[c];
    }
    p.S = 0.0;
    p.dl = 0.0;
    if (FORM == CeTarget::kProbabilities) {
        const float* t = static_cast<const float*>(a.target);
#pragma unroll
        for (int c = 0; c < kCeMaxClasses; ++c) {
            p.wt[c] = c < a.C ? (double)a.w[c] * (double)t[(size_t)c * a.N + pix] : 0.0;
            p.S += p.wt[c];
        }
    } else {
        const long long label = ce_label<FORM>(a.target, pix);
#pragma unroll
        for (int c = 0; c < kCeMaxClasses; ++c) {
            const bool hit = c < a.C && label == c;
            p.wt[c] = hit ? (double)a.w[c] : 0.0;
            if (hit) { p.S = p.wt[c]; p.dl = p.d[c]; }
        }
    }
}

template <CeTarget FORM>
__global__ __launch_bounds__(kAuxThreads) void semantic_ce_forward_kernel(CeArgs a, double* __restrict__ partials) {
    __shared__ double red[kReduceThreads];
    const size_t pix = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    double term = 0.0;
    if (pix < a.N) {
        CePixel p;
        ce_pixel<FORM>(a, pix, p);
        const double log_s = log(p.s);
        if (FORM == CeTarget::kProbabilities) {
#pragma unroll
            for (int c = 0; c < kCeMaxClasses; ++c)
                if (c < a.C) term -= p.wt[c] * (p.d[c] - log_s);   // 0 * (-inf) is NaN, as in torch
        } else {
            term = -p.S * (p.dl - log_s);   // the label's class alone: an -inf logit elsewhere leaves the term finite
        }
    }
    const double sum = block_sum(term, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

template <CeTarget FORM>
__global__ __launch_bounds__(kAuxThreads) void semantic_ce_backward_kernel(CeArgs a, const float* __restrict__ g_loss, float* __restrict__ g_x) {
    const size_t pix = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    if (pix >= a.N) return;
    CePixel p;
    ce_pixel<FORM>(a, pix, p);
    const double k = (double)g_loss[0] / (double)a.N;
#pragma unroll
    for (int c = 0; c < kCeMaxClasses; ++c)
        if (c < a.C) g_x[(size_t)c * a.N + pix] = (float)(k * (p.e[c] / p.s * p.S - p.wt[c]));
}

template <CeTarget FORM>
static hipError_t ce_forward(const CeArgs& a, void* workspace, float* out1, hipStream_t s) {
    double* partials = static_cast<double*>(workspace);
    const int blocks = (int)aux_blocks(a.N);
    hipLaunchKernelGGL(semantic_ce_forward_kernel<FORM>, dim3(blocks), dim3(kAuxThreads), 0, s, a, partials);
    hipLaunchKernelGGL(aux_finalize_kernel<1>, dim3(1), dim3(kReduceThreads), 0, s, partials, blocks, (double)a.N, 1.0, 0.0, out1);
    return hipGetLastError();
}

static hipError_t launch_semantic_ce_forward(const CeArgs& a, CeTarget form, void* workspace, float* out1, hipStream_t s) {
    switch (form) {
        case CeTarget::kProbabilities: return ce_forward<CeTarget::kProbabilities>(a, workspace, out1, s);
        case CeTarget::kLabelsU8: return ce_forward<CeTarget::kLabelsU8>(a, workspace, out1, s);
        case CeTarget::kLabelsI32: return ce_forward<CeTarget::kLabelsI32>(a, workspace, out1, s);
        case CeTarget::kLabelsI64: return ce_forward<CeTarget::kLabelsI64>(a, workspace, out1, s);
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_semantic_ce_backward(const CeArgs& a, CeTarget form, const float* g_loss, float* g_x, hipStream_t s) {
    const dim3 grid((unsigned)aux_blocks(a.N)), block(kAuxThreads);
    switch (form) {
        case CeTarget::kProbabilities: hipLaunchKernelGGL(semantic_ce_backward_kernel<CeTarget::kProbabilities>, grid, block, 0, s, a, g_loss, g_x); break;
        case CeTarget::kLabelsU8: hipLaunchKernelGGL(semantic_ce_backward_kernel<CeTarget::kLabelsU8>, grid, block, 0, s, a, g_loss, g_x); break;
        case CeTarget::kLabelsI32: hipLaunchKernelGGL(semantic_ce_backward_kernel<CeTarget::kLabelsI32>, grid, block, 0, s, a, g_loss, g_x); break;
        case CeTarget::kLabelsI64: hipLaunchKernelGGL(semantic_ce_backward_kernel<CeTarget::kLabelsI64>, grid, block, 0, s, a, g_loss, g_x); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- surface regularisers ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAuxThreads) void surface_reg_forward_kernel(SurfaceRegArgs a, double* __restrict__ partials) {
    __shared__ double red[kReduceThreads];
    const size_t pix = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    double normal = 0.0, dist = 0.0;
    if (pix < a.N) {
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) dot += (double)a.rend_normal[c * a.N + pix] * (double)a.surf_normal[c * a.N + pix];
        normal = 1.0 - dot;
        dist = (double)a.rend_dist[pix];
    }
    const double sum_n = block_sum(normal, red);
    const double sum_d = block_sum(dist, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = sum_n; partials[2 * (size_t)blockIdx.x + 1] = sum_d; }
}

__global__ __launch_bounds__(kAuxThreads) void surface_reg_backward_kernel(SurfaceRegArgs a, const float* __restrict__ g_loss,
                                                                           float* __restrict__ g_rn, float* __restrict__ g_sn,
                                                                           float* __restrict__ g_dist) {
    const size_t pix = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    if (pix >= a.N) return;
    const double g = (double)g_loss[0];
    const double k_n = -(g * a.lambda_normal / (double)a.N);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (g_rn) g_rn[c * a.N + pix] = (float)(k_n * (double)a.surf_normal[c * a.N + pix]);
        if (g_sn) g_sn[c * a.N + pix] = (float)(k_n * (double)a.rend_normal[c * a.N + pix]);
    }
    if (g_dist) g_dist[pix] = (float)(g * a.lambda_dist / (double)a.N);
}

static hipError_t launch_surface_reg_forward(const SurfaceRegArgs& a, void* workspace, float* out3, hipStream_t s) {
    double* partials = static_cast<double*>(workspace);
    const int blocks = (int)aux_blocks(a.N);
    hipLaunchKernelGGL(surface_reg_forward_kernel, dim3(blocks), dim3(kAuxThreads), 0, s, a, partials);
    hipLaunchKernelGGL(aux_finalize_kernel<2>, dim3(1), dim3(kReduceThreads), 0, s, partials, blocks, (double)a.N, a.lambda_normal, a.lambda_dist, out3);
    return hipGetLastError();
}

static hipError_t launch_surface_reg_backward(const SurfaceRegArgs& a, const float* g_loss, float* g_rend_normal, float* g_surf_normal, float* g_rend_dist,
                                       hipStream_t s) {
    hipLaunchKernelGGL(surface_reg_backward_kernel, dim3((unsigned)aux_blocks(a.N)), dim3(kAuxThreads), 0, s, a, g_loss, g_rend_normal, g_surf_normal,
                       g_rend_dist);
    return hipGetLastError();
}

// ---- opacity shrink ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double shrink_sigmoid(float raw) { return 1.0 / (1.0 + exp(-(double)raw)); }

template <bool ACTIVATED>
__global__ __launch_bounds__(kAuxThreads) void opacity_shrink_forward_kernel(size_t P, const float* __restrict__ opacity, double* __restrict__ partials) {
    __shared__ double red[kReduceThreads];
    const size_t i = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    double v = 0.0;
    if (i < P) v = ACTIVATED ? (double)opacity[i] : shrink_sigmoid(opacity[i]);
    const double sum = block_sum(v, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

template <bool ACTIVATED>
__global__ __launch_bounds__(kAuxThreads) void opacity_shrink_backward_kernel(size_t P, const float* __restrict__ opacity, const float* __restrict__ g_loss,
                                                                              float* __restrict__ g_opacity) {
    const size_t i = (size_t)blockIdx.x * kAuxThreads + threadIdx.x;
    if (i >= P) return;
    const double k = (double)g_loss[0] / (double)P;
    if (ACTIVATED) {
        g_opacity[i] = (float)k;
    } else {
        const double s = shrink_sigmoid(opacity[i]);
        g_opacity[i] = (float)(k * (s * (1.0 - s)));
    }
}

static hipError_t launch_opacity_shrink_forward(size_t P, const float* opacity, bool activated, void* workspace, float* out1, hipStream_t s) {
    double* partials = static_cast<double*>(workspace);
    const int blocks = (int)aux_blocks(P);
    if (activated)
        hipLaunchKernelGGL(opacity_shrink_forward_kernel<true>, dim3(blocks), dim3(kAuxThreads), 0, s, P, opacity, partials);
    else
        hipLaunchKernelGGL(opacity_shrink_forward_kernel<false>, dim3(blocks), dim3(kAuxThreads), 0, s, P, opacity, partials);
    hipLaunchKernelGGL(aux_finalize_kernel<1>, dim3(1), dim3(kReduceThreads), 0, s, partials, blocks, (double)P, 1.0, 0.0, out1);
    return hipGetLastError();
}

static hipError_t launch_opacity_shrink_backward(size_t P, const float* opacity, bool activated, const float* g_loss, float* g_opacity, hipStream_t s) {
    const dim3 grid((unsigned)aux_blocks(P)), block(kAuxThreads);
    if (activated)
        hipLaunchKernelGGL(opacity_shrink_backward_kernel<true>, grid, block, 0, s, P, opacity, g_loss, g_opacity);
    else
        hipLaunchKernelGGL(opacity_shrink_backward_kernel<false>, grid, block, 0, s, P, opacity, g_loss, g_opacity);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

namespace {

// shared refusals of the auxiliary losses: the element count, then (forwards only: workspace_bytes != nullptr) the workspace
int aux_count(const char* what, int64_t n, const void* workspace, const size_t* workspace_bytes) {
    if (!aux_loss_supported((size_t)n)) return fail(SR_ERR_UNSUPPORTED, "%s: %lld elements are beyond the launch limits", what, (long long)n);
    if (!workspace_bytes) return SR_OK;
    return check_workspace_size(workspace, *workspace_bytes, aux_loss_workspace_bytes((size_t)n), what);
}

int semantic_ce_args(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                     CeArgs* a, CeTarget* form) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (C < 1 || C > SR_CE_MAX_CLASSES) return fail(SR_ERR_INVALID_ARGUMENT, "%d classes: not in 1..%d", C, SR_CE_MAX_CLASSES);
    if (label_bytes != 0 && label_bytes != 1 && label_bytes != 4 && label_bytes != 8)
        return fail(SR_ERR_INVALID_ARGUMENT, "label_bytes %d: not 0 (probabilities), 1, 4 or 8", label_bytes);
    if (!logits || !target) return fail(SR_ERR_INVALID_ARGUMENT, "logits / target is NULL");
    *form = static_cast<CeTarget>(label_bytes);
    a->C = C;
    a->N = (size_t)W * (size_t)H;
    for (int c = 0; c < kCeMaxClasses; ++c) a->w[c] = c < C ? (weight ? weight[c] : 1.f) : 0.f;
    a->x = logits;
    a->target = target;
    return SR_OK;
}

}  // namespace

extern "C" {

size_t sr_aux_loss_workspace_bytes(int64_t n) { return n > 0 ? aux_loss_workspace_bytes((size_t)n) : 0; }

int sr_semantic_ce_forward(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                           void* workspace, size_t workspace_bytes, float* out1, void* stream) {
    CeArgs a;
    CeTarget form;
    if (int rc = semantic_ce_args(W, H, C, logits, target, label_bytes, weight, &a, &form)) return rc;
    if (!out1) return fail(SR_ERR_INVALID_ARGUMENT, "out1 is NULL");
    if (int rc = aux_count("sr_semantic_ce_forward", (int64_t)a.N, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_semantic_ce_forward(a, form, workspace, out1, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_semantic_ce_backward(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                            const float* g_loss, float* g_logits, void* stream) {
    CeArgs a;
    CeTarget form;
    if (int rc = semantic_ce_args(W, H, C, logits, target, label_bytes, weight, &a, &form)) return rc;
    if (!g_loss || !g_logits) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_logits is NULL");
    if (int rc = aux_count("sr_semantic_ce_backward", (int64_t)a.N, nullptr, nullptr)) return rc;
    SR_HIP(launch_semantic_ce_backward(a, form, g_loss, g_logits, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_surface_reg_forward(int32_t W, int32_t H, const float* rend_normal, const float* surf_normal, const float* rend_dist, double lambda_normal,
                           double lambda_dist, void* workspace, size_t workspace_bytes, float* out3, void* stream) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (!rend_normal || !surf_normal || !rend_dist || !out3) return fail(SR_ERR_INVALID_ARGUMENT, "rend_normal / surf_normal / rend_dist / out3 is NULL");
    const SurfaceRegArgs a{(size_t)W * (size_t)H, lambda_normal, lambda_dist, rend_normal, surf_normal, rend_dist};
    if (int rc = aux_count("sr_surface_reg_forward", (int64_t)a.N, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_surface_reg_forward(a, workspace, out3, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_surface_reg_backward(int32_t W, int32_t H, const float* rend_normal, const float* surf_normal, double lambda_normal, double lambda_dist,
                            const float* g_loss, float* g_rend_normal, float* g_surf_normal, float* g_rend_dist, void* stream) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (!g_loss) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss is NULL");
    if (g_rend_normal && !surf_normal) return fail(SR_ERR_INVALID_ARGUMENT, "g_rend_normal is asked for without surf_normal");
    if (g_surf_normal && !rend_normal) return fail(SR_ERR_INVALID_ARGUMENT, "g_surf_normal is asked for without rend_normal");
    const SurfaceRegArgs a{(size_t)W * (size_t)H, lambda_normal, lambda_dist, rend_normal, surf_normal, nullptr};
    if (int rc = aux_count("sr_surface_reg_backward", (int64_t)a.N, nullptr, nullptr)) return rc;
    if (!g_rend_normal && !g_surf_normal && !g_rend_dist) return SR_OK;
    SR_HIP(launch_surface_reg_backward(a, g_loss, g_rend_normal, g_surf_normal, g_rend_dist, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_opacity_shrink_forward(int64_t P, const float* opacity, int32_t activated, void* workspace, size_t workspace_bytes, float* out1, void* stream) {
    if (P < 1) return fail(SR_ERR_INVALID_ARGUMENT, "P %lld < 1", (long long)P);
    if (!opacity || !out1) return fail(SR_ERR_INVALID_ARGUMENT, "opacity / out1 is NULL");
    if (int rc = aux_count("sr_opacity_shrink_forward", P, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_opacity_shrink_forward((size_t)P, opacity, activated != 0, workspace, out1, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_opacity_shrink_backward(int64_t P, const float* opacity, int32_t activated, const float* g_loss, float* g_opacity, void* stream) {
    if (P < 1) return fail(SR_ERR_INVALID_ARGUMENT, "P %lld < 1", (long long)P);
    if (!g_loss || !g_opacity) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_opacity is NULL");
    if (!activated && !opacity) return fail(SR_ERR_INVALID_ARGUMENT, "opacity is NULL");
    if (int rc = aux_count("sr_opacity_shrink_backward", P, nullptr, nullptr)) return rc;
    SR_HIP(launch_opacity_shrink_backward((size_t)P, opacity, activated != 0, g_loss, g_opacity, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
