// optimizer.hip -- the tail of a training iteration of the reference (train.py:165-200, scene/gaussian_model.py:166-180, 555-557):
//   adam_step_kernel<false>     one launch for up to 8 parameter tensors of a torch.optim.Adam step (no weight decay, no amsgrad)
//   adam_step_kernel<true>      the same step for the rows a per-Gaussian mask selects (the masked re-optimisation model: only the Gaussians
//                               around the removed object move); the other rows are neither read nor written
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
#include "abi.h"

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
    uint32_t row_len;       // adam_step_kernel<true>: elements per row of the mask
};
struct AdamTable {
    AdamSeg seg[SR_ADAM_MAX_SEGMENTS];
    const uint8_t* mask;    // adam_step_kernel<true>: [n / row_len] for every tensor; a row with mask == 0 is neither read nor written
    uint32_t total_chunks;
    float beta2, one_minus_beta1, one_minus_beta2, eps;
};

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamTable& t, float step_size, float bc2_sqrt) {
    m = m + (g - m) * t.one_minus_beta1;
    v = v * t.beta2 + (t.one_minus_beta2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), bc2_sqrt) + t.eps;
    p = p - step_size * __fdiv_rn(m, denom);
}

__device__ __forceinline__ void adam_update_at(const AdamSeg& s, const AdamTable& t, long long i) {
    float pe = s.p[i], me = s.m[i], ve = s.v[i];
    adam_update(pe, s.g[i], me, ve, t, s.step_size, s.bc2_sqrt);
    s.p[i] = pe; s.m[i] = me; s.v[i] = ve;
}

// Where a chunk begins in the rows of the mask.  ROWS = false (the dense step): nothing is computed and every element is selected.
struct AdamChunkRows {
    long long row;   // row of the chunk's first element
    uint32_t col;    // its column
};
template <bool ROWS>
__device__ __forceinline__ AdamChunkRows adam_chunk_rows(const AdamSeg& s, long long base) {
    if (!ROWS) return AdamChunkRows{0, 0u};
    const long long row = base / s.row_len;     // wave-uniform: once per chunk
    return AdamChunkRows{row, (uint32_t)(base - row * s.row_len)};
}
// bit j: element `off + j` of the chunk lies in a selected row, for the first `count` (<= 4) elements behind `off`
template <bool ROWS>
__device__ __forceinline__ uint32_t adam_selected(const AdamSeg& s, const AdamTable& t, AdamChunkRows at, uint32_t off, int count) {
    if (!ROWS) return (1u << count) - 1u;
    const uint32_t x = at.col + off;            // row_len < 2^30 and off < kAdamChunk: no overflow
    uint32_t r = x / s.row_len, c = x - r * s.row_len, bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < count && t.mask[at.row + r] != 0) bits |= 1u << j;
        if (++c == s.row_len) { c = 0; ++r; }
    }
    return bits;
}

// one chunk of a 16-B aligned tensor; FULL: every group of four lies inside the tensor.  A group whose four elements are all selected
// moves as dwordx4; of any other group (the n mod 4 tail; ROWS: a group that straddles a selected and an unselected row) only the
// selected elements are touched, as scalars.
template <bool FULL, bool ROWS>
__device__ __forceinline__ void adam_chunk_vec(const AdamSeg& s, const AdamTable& t, long long base) {
    float4 p[kAdamUnroll], g[kAdamUnroll], m[kAdamUnroll], v[kAdamUnroll];
    long long at[kAdamUnroll];
    uint32_t sel[kAdamUnroll];
    const AdamChunkRows rows = adam_chunk_rows<ROWS>(s, base);
#pragma unroll
    for (int u = 0; u < kAdamUnroll; ++u) {
        const uint32_t off = 4u * (u * kAdamThreads + threadIdx.x);
        at[u] = base + off;
        const long long left = s.n - at[u];
        const int count = (FULL || left >= 4) ? 4 : left > 0 ? (int)left : 0;
        sel[u] = adam_selected<ROWS>(s, t, rows, off, count);
        if (sel[u] == 0xFu) {
            p[u] = *reinterpret_cast<const float4*>(s.p + at[u]);
            g[u] = *reinterpret_cast<const float4*>(s.g + at[u]);
            m[u] = *reinterpret_cast<const float4*>(s.m + at[u]);
            v[u] = *reinterpret_cast<const float4*>(s.v + at[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kAdamUnroll; ++u) {
        if (sel[u] == 0xFu) {
            adam_update(p[u].x, g[u].x, m[u].x, v[u].x, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].y, g[u].y, m[u].y, v[u].y, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].z, g[u].z, m[u].z, v[u].z, t, s.step_size, s.bc2_sqrt);
            adam_update(p[u].w, g[u].w, m[u].w, v[u].w, t, s.step_size, s.bc2_sqrt);
            *reinterpret_cast<float4*>(s.p + at[u]) = p[u];
            *reinterpret_cast<float4*>(s.m + at[u]) = m[u];
            *reinterpret_cast<float4*>(s.v + at[u]) = v[u];
        } else if ((!FULL || ROWS) && sel[u]) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (sel[u] >> j & 1u) adam_update_at(s, t, at[u] + j);
        }
    }
}

// one chunk of a tensor that is only 4-B aligned: consecutive lanes, consecutive elements
template <bool ROWS>
__device__ __forceinline__ void adam_chunk_scalar(const AdamSeg& s, const AdamTable& t, long long base) {
    const AdamChunkRows rows = adam_chunk_rows<ROWS>(s, base);
#pragma unroll 4
    for (int k = 0; k < kAdamChunk / kAdamThreads; ++k) {
        const uint32_t off = k * kAdamThreads + threadIdx.x;
        if (base + off < s.n && adam_selected<ROWS>(s, t, rows, off, 1)) adam_update_at(s, t, base + off);
    }
}

// ROWS: the same step for the rows the table's mask selects (include/surfel_raster.h, sr_adam_step_rows, states when that equals the
// dense step).  (One template, the loop in the kernel itself: behind a reference to the by-value table the segment selects go to scratch.)
template <bool ROWS>
__global__ __launch_bounds__(kAdamThreads) void adam_step_kernel(const AdamTable t) {
    for (uint32_t c = blockIdx.x; c < t.total_chunks; c += gridDim.x) {
        AdamSeg s = t.seg[0];
#pragma unroll
        for (int k = 1; k < SR_ADAM_MAX_SEGMENTS; ++k)
            if (c >= t.seg[k].first_chunk) s = t.seg[k];   // first_chunk ascends; unused slots hold 0xFFFFFFFF
        const long long base = (long long)(c - s.first_chunk) * kAdamChunk;
        if (!s.vec) adam_chunk_scalar<ROWS>(s, t, base);
        else if (base + kAdamChunk <= s.n) adam_chunk_vec<true, ROWS>(s, t, base);
        else adam_chunk_vec<false, ROWS>(s, t, base);
    }
}

namespace {

struct AdamLaunch {
    AdamTable t{};
    int used = 0;
    uint32_t chunks = 0;
    void add(float* p, const float* g, float* m, float* v, long long n, float step_size, float bc2_sqrt, uint32_t row_len) {
        if (n == 0) return;
        AdamSeg& s = t.seg[used++];
        s.p = p; s.g = g; s.m = m; s.v = v;
        s.n = n; s.step_size = step_size; s.bc2_sqrt = bc2_sqrt; s.row_len = row_len;
        s.first_chunk = chunks;
        s.vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
        chunks += (uint32_t)((n + kAdamChunk - 1) / kAdamChunk);
    }
    hipError_t launch(const uint8_t* mask, double beta1, double beta2, double eps, hipStream_t stream) {
        if (chunks == 0) return hipSuccess;
        for (int k = used; k < SR_ADAM_MAX_SEGMENTS; ++k) t.seg[k].first_chunk = 0xFFFFFFFFu;
        t.mask = mask;
        t.total_chunks = chunks;
        t.beta2 = (float)beta2; t.one_minus_beta1 = (float)(1.0 - beta1); t.one_minus_beta2 = (float)(1.0 - beta2); t.eps = (float)eps;
        const uint32_t grid = chunks < (uint32_t)kAdamMaxBlocks ? chunks : (uint32_t)kAdamMaxBlocks;
        if (mask) hipLaunchKernelGGL(adam_step_kernel<true>, dim3(grid), dim3(kAdamThreads), 0, stream, t);
        else hipLaunchKernelGGL(adam_step_kernel<false>, dim3(grid), dim3(kAdamThreads), 0, stream, t);
        return hipGetLastError();
    }
};

template <class Segment>
bool adam_chunks_fit(const Segment* segments, int n_segments) {
    unsigned long long chunks = 0;
    for (int k = 0; k < n_segments; ++k) chunks += ((unsigned long long)segments[k].n + kAdamChunk - 1) / kAdamChunk;
    return chunks < 0x7FFFFFFFull;
}

hipError_t launch_adam_step(const SrAdamSegment* segments, int n_segments, double beta1, double beta2, double eps, hipStream_t stream) {
    AdamLaunch l;
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamSegment& a = segments[k];
        l.add(a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.step_size, a.bc2_sqrt, 1u);
    }
    return l.launch(nullptr, beta1, beta2, eps, stream);
}

hipError_t launch_adam_step_rows(const SrAdamRowSegment* segments, int n_segments, const uint8_t* mask, double beta1, double beta2,
                                 double eps, hipStream_t stream) {
    AdamLaunch l;
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamRowSegment& a = segments[k];
        l.add(a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.step_size, a.bc2_sqrt, (uint32_t)a.row_len);
    }
    return l.launch(mask, beta1, beta2, eps, stream);
}

}  // namespace

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

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the refusals the two Adam calls share: the hyper-parameters ...
static int adam_hyper(double beta1, double beta2, double eps) {
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta1 %g not in [0, 1)", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta2 %g not in [0, 1)", beta2);
    if (!(eps >= 0.0)) return fail(SR_ERR_INVALID_ARGUMENT, "eps %g is negative", eps);
    return SR_OK;
}
// ... and the four arrays of segment k
template <class Segment>
static int adam_pointers(int k, const Segment& a) {
    const void* ptrs[4] = {a.param, a.grad, a.exp_avg, a.exp_avg_sq};
    const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
    for (int j = 0; j < 4; ++j) {
        if (!ptrs[j]) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is NULL", k, names[j]);
        if ((uintptr_t)ptrs[j] & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is not 4-B aligned", k, names[j]);
    }
    return SR_OK;
}

extern "C" {

int sr_adam_step(const SrAdamSegment* segments, int32_t n_segments, double beta1, double beta2, double eps, void* stream) {
    if (!segments) return fail(SR_ERR_INVALID_ARGUMENT, "segments is NULL");
    if (n_segments < 1 || n_segments > SR_ADAM_MAX_SEGMENTS)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_segments %d not in 1..%d", n_segments, SR_ADAM_MAX_SEGMENTS);
    if (int rc = adam_hyper(beta1, beta2, eps)) return rc;
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamSegment& a = segments[k];
        if (a.n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: n %lld is negative", k, (long long)a.n);
        if (int rc = adam_pointers(k, a)) return rc;
    }
    if (!adam_chunks_fit(segments, n_segments)) return fail(SR_ERR_UNSUPPORTED, "the segments hold more than 2^31 chunks of %d elements", SR_ADAM_CHUNK);
    SR_HIP(launch_adam_step(segments, n_segments, beta1, beta2, eps, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_adam_step_rows(const SrAdamRowSegment* segments, int32_t n_segments, int32_t P, const uint8_t* mask, double beta1, double beta2,
                      double eps, void* stream) {
    if (!segments) return fail(SR_ERR_INVALID_ARGUMENT, "segments is NULL");
    if (n_segments < 1 || n_segments > SR_ADAM_MAX_SEGMENTS)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_segments %d not in 1..%d", n_segments, SR_ADAM_MAX_SEGMENTS);
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P > 0 && !mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    if (int rc = adam_hyper(beta1, beta2, eps)) return rc;
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamRowSegment& a = segments[k];
        if (a.row_len < 1 || a.row_len >= (1ll << 30)) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: row_len %lld not in [1, 2^30)", k, (long long)a.row_len);
        if (a.n != (int64_t)P * a.row_len)
            return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: n %lld is not P * row_len = %d * %lld", k, (long long)a.n, P, (long long)a.row_len);
        if (a.n == 0) continue;
        if (int rc = adam_pointers(k, a)) return rc;
    }
    if (P == 0) return SR_OK;
    if (!adam_chunks_fit(segments, n_segments)) return fail(SR_ERR_UNSUPPORTED, "the segments hold more than 2^31 chunks of %d elements", SR_ADAM_CHUNK);
    SR_HIP(launch_adam_step_rows(segments, n_segments, mask, beta1, beta2, eps, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_densification_stats(int32_t P, const float* viewspace_grad, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                           float* max_radii2D, void* stream) {
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P == 0) return SR_OK;
    if (!viewspace_grad) return fail(SR_ERR_INVALID_ARGUMENT, "viewspace_grad is NULL");
    if (!radii) return fail(SR_ERR_INVALID_ARGUMENT, "radii is NULL");
    if (!xyz_gradient_accum) return fail(SR_ERR_INVALID_ARGUMENT, "xyz_gradient_accum is NULL");
    if (!denom) return fail(SR_ERR_INVALID_ARGUMENT, "denom is NULL");
    if (!max_radii2D) return fail(SR_ERR_INVALID_ARGUMENT, "max_radii2D is NULL");
    if (((uintptr_t)viewspace_grad | (uintptr_t)radii | (uintptr_t)xyz_gradient_accum | (uintptr_t)denom | (uintptr_t)max_radii2D) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "viewspace_grad / radii / xyz_gradient_accum / denom / max_radii2D: a pointer is not 4-B aligned");
    hipLaunchKernelGGL(densification_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), P, viewspace_grad, radii,
                       xyz_gradient_accum, denom, max_radii2D);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

}  // extern "C"
