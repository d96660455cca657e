// optimizer.hip -- the tail of a training iteration of the reference (train.py:165-200, scene/gaussian_model.py:166-180, 555-557):
//   adam_step_kernel            one launch for up to 8 parameter tensors of a torch.optim.Adam step (no weight decay, no amsgrad)
//   densification_stats_kernel  xyz_gradient_accum / denom / max_radii2D of the visible Gaussians, without boolean indexing
//
// Adam, per element and in float32, in the order of torch's single-tensor path (this file is built with -ffp-contract=off: the order
// below is what runs; division and square root are the correctly rounded IEEE ones):
//     m     = m + (g - m) * (1 - beta1)
//     v     = v * beta2 + ((1 - beta2) * g) * g
//     denom = sqrt(v) / bc2_sqrt + eps
//     p     = p - step_size * (m / denom)
// step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host (formed in double, rounded to float32), one pair
// per tensor; beta2, 1 - beta1, 1 - beta2 and eps are rounded from the caller's doubles ONCE (1 - float(0.999) is 1.3e-5 away from
// float(0.001): the complement must not be formed from a rounded beta).
//
// The step is a stream over seven arrays (read p, g, m, v; write p, m, v): 28 B per element, no reuse, no LDS, no atomics.  The tensors
// of a launch are cut into chunks of kAdamChunk elements; a workgroup walks chunks grid-stride and finds the tensor of a chunk by a
// search over the (at most 8) first-chunk numbers of the table -- selects over wave-uniform values, no private array, nothing indexed
// with a run-time value.  A tensor whose four pointers are all 16-B aligned moves as dwordx4 (its n mod 4 tail as scalars); one that is
// not moves as coalesced scalars.
#include "launch.h"

namespace sr {

constexpr int kAdamThreads = 256;
constexpr int kAdamUnroll = 4;                                   // independent 16-B groups per thread and array: 16 loads in flight
constexpr int kAdamChunk = kAdamThreads * 4 * kAdamUnroll;       // 4096 elements per workgroup iteration
constexpr int kAdamMaxBlocks = 2048;                             // 256 CUs x 8 workgroups; the rest is grid-strided
static_assert(kAdamChunk == SR_ADAM_CHUNK, "include/surfel_raster.h states the chunk");

struct AdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    float step_size, bc2_sqrt;
    uint32_t first_chunk;   // chunks of the launch in front of this tensor; 0xFFFFFFFF for an unused slot
    uint32_t vec;           // all four pointers 16-B aligned
};
struct AdamTable {
    AdamSeg seg[SR_ADAM_MAX_SEGMENTS];
    uint32_t total_chunks;
    float beta2, one_minus_beta1, one_minus_beta2, eps;
};

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamTable& t, float step_size, float bc2_sqrt) {
    m = m + (g - m) * t.one_minus_beta1;
    v = v * t.beta2 + (t.one_minus_beta2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), bc2_sqrt) + t.eps;
    p = p - step_size * __fdiv_rn(m, denom);
}

// one chunk of a 16-B aligned tensor; FULL: every group of four lies inside the tensor
template <bool FULL>
__device__ __forceinline__ void adam_chunk_vec(const AdamSeg& s, const AdamTable& t, long long base) {
    float4 p[kAdamUnroll], g[kAdamUnroll], m[kAdamUnroll], v[kAdamUnroll];
    long long at[kAdamUnroll];
#pragma unroll
    for (int u = 0; u < kAdamUnroll; ++u) {
        at[u] = base + 4ll * (u * kAdamThreads + (int)threadIdx.x);
        if (FULL || at[u] + 4 <= s.n) {
            p[u] = *reinterpret_cast<const float4*>(s.p + at[u]);
            g[u] = *reinterpret_cast<const float4*>(s.g + at[u]);
            m[u] = *reinterpret_cast<const float4*>(s.m + at[u]);
            v[u] = *reinterpret_cast<const float4*>(s.v + at[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kAdamUnroll; ++u) {
        if (FULL || at[u] + 4 <= s.n) {
            adam_update(p[u].x, g[u].x, m[u].x, v[u].x, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].y, g[u].y, m[u].y, v[u].y, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].z, g[u].z, m[u].z, v[u].z, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].w, g[u].w, m[u].w, v[u].w, t, s.step_size, s.bc2_sqrt);
            *reinterpret_cast<float4*>(s.p + at[u]) = p[u];
            *reinterpret_cast<float4*>(s.m + at[u]) = m[u];
            *reinterpret_cast<float4*>(s.v + at[u]) = v[u];
        } else {
            for (long long i = at[u]; i < s.n; ++i) {   // the n mod 4 tail: one thread, at most three elements
                float pe = s.p[i], me = s.m[i], ve = s.v[i];
                adam_update(pe, s.g[i], me, ve, t, s.step_size, s.bc2_sqrt);
                s.p[i] = pe; s.m[i] = me; s.v[i] = ve;
            }
        }
    }
}

// one chunk of a tensor that is only 4-B aligned: consecutive lanes, consecutive elements
__device__ __forceinline__ void adam_chunk_scalar(const AdamSeg& s, const AdamTable& t, long long base) {
#pragma unroll 4
    for (int k = 0; k < kAdamChunk / kAdamThreads; ++k) {
        const long long i = base + k * kAdamThreads + (int)threadIdx.x;
        if (i < s.n) {
            float pe = s.p[i], me = s.m[i], ve = s.v[i];
            adam_update(pe, s.g[i], me, ve, t, s.step_size, s.bc2_sqrt);
            s.p[i] = pe; s.m[i] = me; s.v[i] = ve;
        }
    }
}

__global__ __launch_bounds__(kAdamThreads) void adam_step_kernel(const AdamTable t) {
    for (uint32_t c = blockIdx.x; c < t.total_chunks; c += gridDim.x) {
        AdamSeg s = t.seg[0];
#pragma unroll
        for (int k = 1; k < SR_ADAM_MAX_SEGMENTS; ++k)
            if (c >= t.seg[k].first_chunk) s = t.seg[k];   // first_chunk ascends; unused slots hold 0xFFFFFFFF
        const long long base = (long long)(c - s.first_chunk) * kAdamChunk;
        if (!s.vec) adam_chunk_scalar(s, t, base);
        else if (base + kAdamChunk <= s.n) adam_chunk_vec<true>(s, t, base);
        else adam_chunk_vec<false>(s, t, base);
    }
}

bool adam_supported(const SrAdamSegment* segments, int n_segments) {
    unsigned long long chunks = 0;
    for (int k = 0; k < n_segments; ++k) chunks += ((unsigned long long)segments[k].n + kAdamChunk - 1) / kAdamChunk;
    return chunks < 0x7FFFFFFFull;
}

hipError_t launch_adam_step(const SrAdamSegment* segments, int n_segments, double beta1, double beta2, double eps, hipStream_t stream) {
    AdamTable t{};
    uint32_t chunks = 0;
    int used = 0;
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamSegment& a = segments[k];
        if (a.n == 0) continue;
        AdamSeg& s = t.seg[used++];
        s.p = a.param; s.g = a.grad; s.m = a.exp_avg; s.v = a.exp_avg_sq;
        s.n = a.n; s.step_size = a.step_size; s.bc2_sqrt = a.bc2_sqrt;
        s.first_chunk = chunks;
        s.vec = (((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15u) == 0;
        chunks += (uint32_t)((a.n + kAdamChunk - 1) / kAdamChunk);
    }
    if (chunks == 0) return hipSuccess;
    for (int k = used; k < SR_ADAM_MAX_SEGMENTS; ++k) t.seg[k].first_chunk = 0xFFFFFFFFu;
    t.total_chunks = chunks;
    t.beta2 = (float)beta2; t.one_minus_beta1 = (float)(1.0 - beta1); t.one_minus_beta2 = (float)(1.0 - beta2); t.eps = (float)eps;
    const uint32_t grid = chunks < (uint32_t)kAdamMaxBlocks ? chunks : (uint32_t)kAdamMaxBlocks;
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(kAdamThreads), 0, stream, t);
    return hipGetLastError();
}

// [REF train.py:168-169, scene/gaussian_model.py:555-557] with visibility_filter = radii > 0: rows of invisible Gaussians are neither
// read (their gradient row may hold anything) nor written.
__global__ __launch_bounds__(256) void densification_stats_kernel(int P, const float* __restrict__ viewspace_grad, const int* __restrict__ radii,
                                                                  float* __restrict__ xyz_gradient_accum, float* __restrict__ denom,
                                                                  float* __restrict__ max_radii2D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = viewspace_grad[3 * (size_t)i], gy = viewspace_grad[3 * (size_t)i + 1], gz = viewspace_grad[3 * (size_t)i + 2];
    xyz_gradient_accum[i] += __fsqrt_rn(gx * gx + gy * gy + gz * gz);
    denom[i] += 1.f;
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

hipError_t launch_densification_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum, float* denom,
                                      float* max_radii2D, hipStream_t stream) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(densification_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, viewspace_grad, radii,
                       xyz_gradient_accum, denom, max_radii2D);
    return hipGetLastError();
}

}  // namespace sr
