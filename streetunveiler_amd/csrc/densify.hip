// densify.hip -- the densify-and-prune step of the reference (scene/gaussian_model.py:402-553: densify_and_prune, densify_and_clone,
// densify_and_split, densification_postfix, cat_tensors_to_optimizer, _prune_optimizer, prune_points) as one decision pass, one scan
// and one gather (include/surfel_raster.h states the semantics):
//   densify_decide_kernel   one thread per Gaussian: the flag byte (clone, split, keep-self, keep-child) + the four counts of its block
//   densify_totals_kernel   exclusive scan of the block counts (one block); the four totals go to the host's pinned words
//   densify_map_kernel      the scans inside each block again, from the flag bytes: every OUTPUT row's source index and kind
//   densify_gather_kernel   up to 8 tensors per launch, each walked as a flat stream of 32-bit output words
// No atomics anywhere: equal inputs give equal bits.  Built with -ffp-contract=off: the order of the child position and the child scale
// below is the one that runs; the quotient accum / denom, 1 / norm and exp(s) / 1.6 are correctly rounded IEEE divisions.
#include <cmath>

#include "abi.h"
#include "scan.h"

namespace sr {

constexpr int kDfThreads = 256;               // Gaussians per block of the decision and the map kernel
constexpr int kDfChunkWords = 4096;           // output words of one tensor a workgroup of the gather handles per iteration
constexpr int kDfMaxBlocks = 4096;            // 256 CUs x 16 workgroups; the rest is grid-strided
constexpr uint32_t kDfIndexMask = 0x3FFFFFFFu;

struct DensifyRule {   // a kernel parameter, by value
    float max_grad, min_opacity, percent_dense_extent, ws_limit;   // ws_limit < 0: no world-size test
    int select;        // 0: nothing is clone- or split-selected and accum / denom are not read (max_grad is +inf or NaN)
};

struct DensifyLayout {
    size_t flags, map, child_rank, totals, total;
    int nblocks;
};
static DensifyLayout densify_layout(int P) {
    DensifyLayout L;
    const size_t n = P > 0 ? (size_t)P : 0;
    L.nblocks = (int)((n + kDfThreads - 1) / kDfThreads);
    Carver c;
    L.flags = c.take(n);
    L.map = c.take(8 * n);
    L.child_rank = c.take(4 * n);
    L.totals = c.take(16 * ((size_t)L.nblocks + 1));
    L.total = c.off;
    return L;
}
static size_t densify_workspace_bytes(int P) { return densify_layout(P).total; }

// ---- decision ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float max_like_torch(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }   // torch.max keeps a NaN
__device__ __forceinline__ float child_scale(float s) { return logf(__fdiv_rn(expf(s), 1.6f)); }

__device__ __forceinline__ uint32_t densify_flags(int i, const float* __restrict__ accum, const float* __restrict__ denom,
                                                  const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                  const uint8_t* __restrict__ prune_mask, const DensifyRule& r) {
    bool clone_selected = false, split_selected = false;   // [REF] the clone tests torch.norm(grads), the split the signed padded_grad
    if (r.select) {
        float g = __fdiv_rn(accum[i], denom[i]);
        if (g != g) g = 0.f;
        clone_selected = fabsf(g) >= r.max_grad;
        split_selected = g >= r.max_grad;
    }
    const float s0 = scaling[2 * (size_t)i], s1 = scaling[2 * (size_t)i + 1];
    const float big = max_like_torch(expf(s0), expf(s1));
    const bool clone = clone_selected && big <= r.percent_dense_extent;
    const bool split = split_selected && big > r.percent_dense_extent;
    const float alpha = __fdiv_rn(1.f, 1.f + expf(-opacity[i]));
    const bool pruned = alpha < r.min_opacity || (prune_mask && prune_mask[i]);
    const bool world = r.ws_limit >= 0.f;
    const bool self_pruned = pruned || (world && big > r.ws_limit);
    const float child_big = max_like_torch(expf(child_scale(s0)), expf(child_scale(s1)));
    const bool child_pruned = pruned || (world && child_big > r.ws_limit);
    return (clone ? SR_DENSIFY_FLAG_CLONE : 0u) | (split ? SR_DENSIFY_FLAG_SPLIT : 0u) |
           (!split && !self_pruned ? SR_DENSIFY_FLAG_KEEP_SELF : 0u) | (split && !child_pruned ? SR_DENSIFY_FLAG_KEEP_CHILD : 0u);
}

// the four things that are counted, one byte each: kept originals | kept clones | split-selected | kept child pairs (a wave holds 64)
__device__ __forceinline__ uint32_t packed_counts(uint32_t f) {
    const uint32_t keep = (f >> 2) & 1u;
    return keep | ((keep & f) << 8) | (((f >> 1) & 1u) << 16) | (((f >> 3) & 1u) << 24);
}
__device__ __forceinline__ uint4 unpack_counts(uint32_t p) { return make_uint4(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u, p >> 24); }
// The scan of the packed word inside a wave, its four counts across the waves (a block holds 256: a byte would overflow): the exclusive
// prefix of the four counts over the block + the block's totals
__device__ __forceinline__ uint4 block_exclusive_counts(uint32_t packed, uint4* s_w, uint4& total) {
    return block_exclusive_from_waves<kDfThreads / 64>(unpack_counts(wave_inclusive_scan(packed)), unpack_counts(packed), s_w, total);
}

__global__ __launch_bounds__(kDfThreads) void densify_decide_kernel(int P, const float* __restrict__ accum, const float* __restrict__ denom,
                                                                    const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                                    const uint8_t* __restrict__ prune_mask, const DensifyRule rule,
                                                                    uint8_t* __restrict__ flags, uint4* __restrict__ block_total) {
    __shared__ uint4 s_w[kDfThreads / 64];
    const int tid = threadIdx.x, i = blockIdx.x * kDfThreads + tid;
    uint32_t f = 0;
    if (i < P) {
        f = densify_flags(i, accum, denom, opacity, scaling, prune_mask, rule);
        flags[i] = (uint8_t)f;
    }
    uint4 total;
    block_exclusive_counts(packed_counts(f), s_w, total);   // (only the totals are used)
    if (tid == 0) block_total[blockIdx.x] = total;
}

// exclusive scan of block_total[0 .. nblocks) in place, one block; block_total[nblocks] = the four totals, also stored straight into the
// caller's pinned host words when given
__global__ __launch_bounds__(kDfThreads) void densify_totals_kernel(uint4* __restrict__ block_total, int nblocks, uint4* __restrict__ total_host) {
    __shared__ uint4 s_w[kDfThreads / 64];
    const uint4 total = carried_exclusive_scan<kDfThreads / 64>(block_total, nblocks, s_w);
    if (threadIdx.x == 0) {
        block_total[nblocks] = total;
        if (total_host) *total_host = total;
    }
}

__global__ __launch_bounds__(kDfThreads) void densify_map_kernel(int P, const uint8_t* __restrict__ flags, const uint4* __restrict__ block_base,
                                                                 int nblocks, uint32_t* __restrict__ map, uint32_t* __restrict__ child_rank) {
    __shared__ uint4 s_w[kDfThreads / 64];
    const int tid = threadIdx.x, i = blockIdx.x * kDfThreads + tid;
    const uint32_t f = i < P ? flags[i] : 0u;
    uint4 block_counts;   // (not used: the totals of all blocks are what places the output rows)
    const uint4 at = block_base[blockIdx.x] + block_exclusive_counts(packed_counts(f), s_w, block_counts);
    const uint4 total = block_base[nblocks];   // K, C, S, H
    if (f & SR_DENSIFY_FLAG_KEEP_SELF) {
        map[at.x] = (uint32_t)i;
        if (f & SR_DENSIFY_FLAG_CLONE) map[total.x + at.y] = (uint32_t)i | ((uint32_t)SR_DENSIFY_KIND_CLONE << 30);
    }
    if (f & SR_DENSIFY_FLAG_KEEP_CHILD) {
        const uint32_t first = total.x + total.y + at.w;
        map[first] = (uint32_t)i | ((uint32_t)SR_DENSIFY_KIND_CHILD0 << 30);
        map[first + total.w] = (uint32_t)i | ((uint32_t)SR_DENSIFY_KIND_CHILD1 << 30);
        child_rank[at.w] = at.z;
    }
}

static hipError_t densify_plan(int P, const float* accum, const float* denom, const float* opacity, const float* scaling, const DensifyRule& rule,
                        const uint8_t* prune_mask, void* workspace, uint32_t* counts_pinned_dev, hipStream_t s) {
    const DensifyLayout L = densify_layout(P);
    uint8_t* flags = at<uint8_t>(workspace, L.flags);
    uint4* totals = at<uint4>(workspace, L.totals);
    hipLaunchKernelGGL(densify_decide_kernel, dim3(L.nblocks), dim3(kDfThreads), 0, s, P, accum, denom, opacity, scaling, prune_mask, rule, flags, totals);
    hipLaunchKernelGGL(densify_totals_kernel, dim3(1), dim3(kDfThreads), 0, s, totals, L.nblocks, reinterpret_cast<uint4*>(counts_pinned_dev));
    hipLaunchKernelGGL(densify_map_kernel, dim3(L.nblocks), dim3(kDfThreads), 0, s, P, flags, totals, L.nblocks,
                       at<uint32_t>(workspace, L.map), at<uint32_t>(workspace, L.child_rank));
    return hipGetLastError();
}

static const uint32_t* densify_counts_device(int P, const void* workspace) {
    const DensifyLayout L = densify_layout(P);
    return reinterpret_cast<const uint32_t*>(static_cast<const char*>(workspace) + L.totals + 16 * (size_t)L.nblocks);
}

// ---- gather --------------------------------------------------------------------------------------------------------------------------
struct GatherSeg {
    const uint32_t* src;
    uint32_t* dst;
    uint32_t row_words;
    uint32_t magic;            // floor(2^32 / row_words) + 1: __umulhi(e, magic) == e / row_words for e < 65536 (row_words >= 2)
    uint32_t role;
    uint32_t rows_per_chunk;
    uint32_t first_chunk;      // chunks of the launch in front of this tensor; 0xFFFFFFFF for an unused slot
};
struct GatherTable {
    GatherSeg seg[SR_DENSIFY_MAX_SEGMENTS];
    uint32_t total_chunks;
    uint32_t rows_out;         // K + C + 2 H
    uint32_t child_base;       // K + C: the output row of the first child
    uint32_t n_split, n_child; // S, H
    const uint32_t* map;
    const uint32_t* child_rank;
    const float* noise;
    const float* rotation;
    const float* scaling;
};

// [REF densify_and_split + utils/general_utils.py build_rotation] component `col` of R(q / |q|) (exp(s0) n0, exp(s1) n1, 0) + xyz
__device__ __forceinline__ float child_position(const GatherTable& t, const float* __restrict__ xyz, uint32_t parent, uint32_t child, uint32_t row,
                                                uint32_t col) {
    const uint32_t j = t.child_rank[row - t.child_base - child * t.n_child];
    const size_t at = 2 * ((size_t)child * t.n_split + j);
    const float v0 = expf(t.scaling[2 * (size_t)parent]) * t.noise[at], v1 = expf(t.scaling[2 * (size_t)parent + 1]) * t.noise[at + 1];
    const float* q = t.rotation + 4 * (size_t)parent;
    const float norm = __fsqrt_rn(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = __fdiv_rn(q[0], norm), x = __fdiv_rn(q[1], norm), y = __fdiv_rn(q[2], norm), z = __fdiv_rn(q[3], norm);
    float a, b;
    if (col == 0) { a = 1.f - 2.f * (y * y + z * z); b = 2.f * (x * y - r * z); }
    else if (col == 1) { a = 2.f * (x * y + r * z); b = 1.f - 2.f * (x * x + z * z); }
    else { a = 2.f * (x * z - r * y); b = 2.f * (y * z + r * x); }
    return (a * v0 + b * v1) + xyz[3 * (size_t)parent + col];
}

__global__ __launch_bounds__(kDfThreads) void densify_gather_kernel(const GatherTable t) {
    for (uint32_t c = blockIdx.x; c < t.total_chunks; c += gridDim.x) {
        GatherSeg s = t.seg[0];
#pragma unroll
        for (int k = 1; k < SR_DENSIFY_MAX_SEGMENTS; ++k)
            if (c >= t.seg[k].first_chunk) s = t.seg[k];   // first_chunk ascends; unused slots hold 0xFFFFFFFF
        const uint32_t row0 = (c - s.first_chunk) * s.rows_per_chunk;
        const uint32_t left = t.rows_out - row0;
        const uint32_t n = (left < s.rows_per_chunk ? left : s.rows_per_chunk) * s.row_words;   // < 65536
        uint32_t* __restrict__ out = s.dst + (size_t)row0 * s.row_words;
        for (uint32_t e = threadIdx.x; e < n; e += kDfThreads) {
            const uint32_t local = s.row_words == 1u ? e : __umulhi(e, s.magic);
            const uint32_t col = e - local * s.row_words;
            const uint32_t m = t.map[row0 + local];
            const uint32_t parent = m & kDfIndexMask, kind = m >> 30;
            uint32_t value;
            if (kind == SR_DENSIFY_KIND_ORIGINAL || s.role == SR_DENSIFY_ROLE_COPY || (kind == SR_DENSIFY_KIND_CLONE && s.role != SR_DENSIFY_ROLE_MOMENT))
                value = s.src[(size_t)parent * s.row_words + col];
            else if (s.role == SR_DENSIFY_ROLE_MOMENT)
                value = 0u;
            else if (s.role == SR_DENSIFY_ROLE_SCALING)
                value = __float_as_uint(child_scale(__uint_as_float(s.src[(size_t)parent * s.row_words + col])));
            else
                value = __float_as_uint(child_position(t, reinterpret_cast<const float*>(s.src), parent, kind - SR_DENSIFY_KIND_CHILD0, row0 + local, col));
            out[e] = value;
        }
    }
}

static hipError_t densify_apply(int P, const uint32_t* counts, const float* noise, const float* rotation, const float* scaling,
                         const SrDensifySegment* segments, int n_segments, const void* workspace, hipStream_t stream) {
    const DensifyLayout L = densify_layout(P);
    const char* ws = static_cast<const char*>(workspace);
    GatherTable t{};
    t.rows_out = counts[0] + counts[1] + 2 * counts[3];
    t.child_base = counts[0] + counts[1];
    t.n_split = counts[2];
    t.n_child = counts[3];
    t.map = reinterpret_cast<const uint32_t*>(ws + L.map);
    t.child_rank = reinterpret_cast<const uint32_t*>(ws + L.child_rank);
    t.noise = noise; t.rotation = rotation; t.scaling = scaling;
    unsigned long long chunks = 0;
    int used = 0;
    for (int k = 0; k < n_segments && t.rows_out > 0; ++k) {
        const SrDensifySegment& a = segments[k];
        if (a.row_words == 0) continue;
        GatherSeg& s = t.seg[used++];
        s.src = static_cast<const uint32_t*>(a.src);
        s.dst = static_cast<uint32_t*>(a.dst);
        s.row_words = (uint32_t)a.row_words;
        s.magic = a.row_words >= 2 ? (uint32_t)(0x100000000ull / (uint32_t)a.row_words) + 1u : 0u;
        s.role = (uint32_t)a.role;
        s.rows_per_chunk = a.row_words <= kDfChunkWords ? (uint32_t)(kDfChunkWords / a.row_words) : 1u;
        s.first_chunk = (uint32_t)chunks;
        chunks += (t.rows_out + s.rows_per_chunk - 1) / s.rows_per_chunk;
    }
    if (chunks == 0) return hipSuccess;
    if (chunks >= 0xFFFFFFFFull) return hipErrorInvalidValue;   // (8 tensors of 2^31 rows: beyond P < 2^30)
    for (int k = used; k < SR_DENSIFY_MAX_SEGMENTS; ++k) t.seg[k].first_chunk = 0xFFFFFFFFu;
    t.total_chunks = (uint32_t)chunks;
    const uint32_t grid = t.total_chunks < (uint32_t)kDfMaxBlocks ? t.total_chunks : (uint32_t)kDfMaxBlocks;
    hipLaunchKernelGGL(densify_gather_kernel, dim3(grid), dim3(kDfThreads), 0, stream, t);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

extern "C" {

size_t sr_densify_workspace_bytes(int32_t P) { return densify_workspace_bytes(P > 0 ? P : 0); }

int sr_densify_plan(int32_t P, const float* accum, const float* denom, const float* opacity, const float* scaling, float max_grad,
                    float min_opacity, float percent_dense_extent, float ws_limit, const uint8_t* prune_mask, void* workspace,
                    size_t workspace_bytes, uint32_t* counts_out, void* stream) {
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (!counts_out) return fail(SR_ERR_INVALID_ARGUMENT, "counts_out is NULL");
    counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
    if (P == 0) return SR_OK;
    if (P >= (1 << 30)) return fail(SR_ERR_UNSUPPORTED, "P = %d: the source map holds 30-bit indices", P);
    DensifyRule rule{max_grad, min_opacity, percent_dense_extent, ws_limit, max_grad < INFINITY ? 1 : 0};   // (NaN: not below +inf)
    if (rule.select && (!accum || !denom)) return fail(SR_ERR_INVALID_ARGUMENT, "accum / denom is NULL (only a max_grad of +inf goes without them)");
    if (!opacity || !scaling) return fail(SR_ERR_INVALID_ARGUMENT, "opacity / scaling is NULL");
    if (int rc = check_workspace(workspace, workspace_bytes, densify_workspace_bytes(P))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // K, C, S and H travel like sr_forward_plan's D: the totals kernel stores them into the calling thread's pinned words when those are
    // mapped into the device's address space, else a DMA copy fetches them; the host waits for the stream once.
    uint32_t* pinned = pinned_words();
    uint32_t* pinned_dev = nullptr;
    if (pinned && hipHostGetDevicePointer(reinterpret_cast<void**>(&pinned_dev), pinned, 0) != hipSuccess) { pinned_dev = nullptr; (void)hipGetLastError(); }
    SR_HIP(densify_plan(P, accum, denom, opacity, scaling, rule, prune_mask, workspace, pinned_dev ? pinned_dev + 4 : nullptr, s));
    uint32_t* target = pinned ? pinned + 4 : counts_out;
    if (!pinned_dev) SR_HIP(hipMemcpyAsync(target, densify_counts_device(P, workspace), 16, hipMemcpyDeviceToHost, s));
    SR_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) counts_out[k] = reinterpret_cast<volatile uint32_t*>(target)[k];
    return SR_OK;
}

int sr_densify_apply(int32_t P, const uint32_t* counts, const float* noise, const float* rotation, const float* scaling,
                     const SrDensifySegment* segments, int32_t n_segments, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if (n_segments < 0 || n_segments > SR_DENSIFY_MAX_SEGMENTS)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_segments %d not in 0..%d", n_segments, SR_DENSIFY_MAX_SEGMENTS);
    if (n_segments > 0 && !segments) return fail(SR_ERR_INVALID_ARGUMENT, "segments is NULL");
    const uint64_t K = counts[0], C = counts[1], S = counts[2], H = counts[3];
    if (C > K || H > S || K + S > (uint64_t)P)
        return fail(SR_ERR_INVALID_ARGUMENT, "counts {%u, %u, %u, %u} are not those of a plan over %d Gaussians", counts[0], counts[1], counts[2], counts[3], P);
    const bool rows = K + C + 2 * H > 0;
    for (int k = 0; k < n_segments; ++k) {
        const SrDensifySegment& a = segments[k];
        if (a.role < SR_DENSIFY_ROLE_COPY || a.role > SR_DENSIFY_ROLE_SCALING) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: unknown role %d", k, a.role);
        if (a.row_words < 0 || a.row_words > 65535) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: row_words %d not in 0..65535", k, a.row_words);
        if (a.role == SR_DENSIFY_ROLE_XYZ && a.row_words != 3) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: the xyz role takes rows of 3 words, not %d", k, a.row_words);
        if (a.role == SR_DENSIFY_ROLE_SCALING && a.row_words != 2) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: the scaling role takes rows of 2 words, not %d", k, a.row_words);
        if (a.row_words == 0 || !rows) continue;
        if (!a.src || !a.dst) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: src / dst is NULL", k);
        if (((uintptr_t)a.src | (uintptr_t)a.dst) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: src / dst is not 4-B aligned", k);
        if (a.role == SR_DENSIFY_ROLE_XYZ && H > 0 && (!noise || !rotation || !scaling))
            return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: the xyz role needs noise, rotation and scaling when children survive", k);
    }
    if (P == 0 || !rows || n_segments == 0) return SR_OK;
    if (int rc = check_workspace_size(workspace, workspace_bytes, densify_workspace_bytes(P))) return rc;   // (no alignment test here, unlike the plan)
    SR_HIP(densify_apply(P, counts, noise, rotation, scaling, segments, n_segments, workspace, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
