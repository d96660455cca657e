// K-nearest-neighbour mean squared distance == `dist3knn` / `dist10knn` / `meanDistFromReferencePcd` of the
// reference's simple-knn fork [REF /root/reference/scene/gaussian_model.py:16,151; scene/mask_gaussian.py:21;
// inpainting_pipeline/2_condition_preparation/2_generate_inpainted_mask.py:27,71-73].  The fork's source is an un-vendored
// submodule (/root/reference/.gitmodules: submodules/simple-knn, no pinned SHA); what is restated is the published
// simple-knn algorithm it descends from: out[i] = mean of the K smallest SQUARED distances from point i to the other points.
//
// The search is exact.  Points are ordered along a 30-bit Morton curve (hand-written radix sort, radix_sort.hip), cut into
// boxes of 512 consecutive points with their AABBs, and one wave64 handles 64 curve-consecutive queries: lanes test 64 boxes
// at a time against the wave's query AABB and its current worst K-th distance (ballot), and every surviving box is scanned
// by all lanes together -- the candidate is wave-uniform (scalar loads), the distance and the branch-free K-best insertion
// run per lane, so there is no divergence and no LDS.  Integer/bandwidth/VALU work only; no MFMA.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "cloud.h"
#include "abi.h"

namespace sr {

constexpr int kKnnThreads = 256;

// ---- ordering a cloud ---------------------------------------------------------------------------------------
// Bounds, Morton codes, the sorted (x, y, z, index) array and the box AABBs are what cluster.hip searches too (launch.h: cloud_order and
// its neighbours).  Its clouds carry a mask -- kMasked: a point takes part when active[i] != 0 (active == nullptr: every point) and its
// coordinates are finite.  A point that does not is left out of the bounds, gets kDeadCode, which the 31-bit sort puts behind every
// live point of the curve, and is stored as (inf, inf, inf) like a non-finite point of the kNN.  The kNN's own instantiations
// (kMasked = false) are the kernels they were.
constexpr uint32_t kDeadCode = 1u << 30;

template <bool kMasked>
__device__ __forceinline__ bool takes_part(const float* __restrict__ pts, const uint8_t* __restrict__ active, size_t i) {
    if (!kMasked) return true;
    if (active && !active[i]) return false;
    return fabsf(pts[3 * i]) <= FLT_MAX && fabsf(pts[3 * i + 1]) <= FLT_MAX && fabsf(pts[3 * i + 2]) <= FLT_MAX;   // false for NaN too
}

template <bool kMasked>
__global__ __launch_bounds__(kKnnThreads) void knn_bounds_partial_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ active, int n,
                                                                          float* __restrict__ partial) {
    __shared__ float s_red[6][kKnnThreads / kWave];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * kKnnThreads + threadIdx.x; i < n; i += gridDim.x * kKnnThreads) {
        if (!takes_part<kMasked>(pts, active, (size_t)i)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = pts[3 * (size_t)i + c]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int o = kWave / 2; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_red[c][wave] = lo[c]; s_red[3 + c][wave] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s_red[threadIdx.x][0];
        for (int w = 1; w < kKnnThreads / kWave; ++w) v = threadIdx.x < 3 ? fminf(v, s_red[threadIdx.x][w]) : fmaxf(v, s_red[threadIdx.x][w]);
        partial[blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ void knn_bounds_final_kernel(const float* __restrict__ partial, int rows, float* __restrict__ bounds) {
    const int c = threadIdx.x;
    if (c >= 6) return;
    float v = partial[c];
    for (int r = 1; r < rows; ++r) v = c < 3 ? fminf(v, partial[r * 6 + c]) : fmaxf(v, partial[r * 6 + c]);
    bounds[c] = v;
}

// ---- Morton codes -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

template <bool kMasked>
__global__ void knn_morton_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ active, int n, const float* __restrict__ bounds,
                                  uint32_t* __restrict__ codes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!takes_part<kMasked>(pts, active, (size_t)i)) { codes[i] = kDeadCode; return; }
    uint32_t q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = bounds[c], ext = fmaxf(bounds[3 + c] - lo, 1e-30f);
        const float t = (pts[3 * (size_t)i + c] - lo) / ext * 1023.f;
        q[c] = (uint32_t)fminf(fmaxf(t, 0.f), 1023.f);   // NaN -> 0
    }
    codes[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
}

// sorted[i] = (x, y, z, original index) of the i-th point along the curve.
// A point with a NaN or inf coordinate is nobody's neighbour and has none, as in the oracle, whose `d < best` never takes its NaN / inf
// distance.  It is stored as (inf, inf, inf): its distance to every finite point is then +inf, which the fminf / fmaxf chain of insert_best
// carries through and drops, and never NaN, for which both calls hand back best[k] and duplicate every entry one slot down.  The search
// kernel switches such a query off (`live`), the box kernel leaves it out of the AABBs; the scan loop pays nothing for it.
template <bool kMasked>
__global__ void knn_gather_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ active, const uint32_t* __restrict__ order, int n,
                                  float4* __restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = order[i];
    const float x = pts[3 * (size_t)j], y = pts[3 * (size_t)j + 1], z = pts[3 * (size_t)j + 2];
    const bool finite = fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX && !(kMasked && active && !active[j]);   // false for NaN too
    sorted[i] = finite ? make_float4(x, y, z, __uint_as_float(j)) : make_float4(INFINITY, INFINITY, INFINITY, __uint_as_float(j));
}

// AABB of each run of kKnnBox curve-consecutive points: boxes[2b] = (min, -), boxes[2b+1] = (max, -)
__global__ __launch_bounds__(kKnnThreads) void knn_boxes_kernel(const float4* __restrict__ sorted, int n, float4* __restrict__ boxes) {
    __shared__ float s_red[6][kKnnThreads / kWave];
    const int base = blockIdx.x * kKnnBox;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int j = threadIdx.x; j < kKnnBox && base + j < n; j += kKnnThreads) {
        const float4 p = sorted[base + j];
        if (!(p.x <= FLT_MAX)) continue;   // a non-finite point (knn_gather_kernel): no candidate, so no part of the box
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int o = kWave / 2; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_red[c][wave] = lo[c]; s_red[3 + c][wave] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kKnnThreads / kWave; ++w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { s_red[c][0] = fminf(s_red[c][0], s_red[c][w]); s_red[3 + c][0] = fmaxf(s_red[3 + c][0], s_red[3 + c][w]); }
        }
        boxes[2 * blockIdx.x] = make_float4(s_red[0][0], s_red[1][0], s_red[2][0], 0.f);
        boxes[2 * blockIdx.x + 1] = make_float4(s_red[3][0], s_red[4][0], s_red[5][0], 0.f);
    }
}

// ---- search --------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void insert_best(float (&best)[K], float d) {   // keeps best[] ascending; branch-free; d is never NaN (knn_gather_kernel)
#pragma unroll
    for (int k = 0; k < K; ++k) { const float lo = fminf(best[k], d); d = fmaxf(best[k], d); best[k] = lo; }
}

// kSelf: queries ARE the reference points (same sorted array); a point is not its own neighbour.
template <int K, bool kSelf>
__global__ __launch_bounds__(kKnnThreads) void knn_search_kernel(const float4* __restrict__ q_sorted, int nq,
                                                                  const float4* __restrict__ r_sorted, const uint32_t* __restrict__ r_codes,
                                                                  const uint32_t* __restrict__ q_codes, int nr,
                                                                  const float4* __restrict__ boxes, int n_boxes, int take_sqrt,
                                                                  float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_base = (blockIdx.x * (kKnnThreads / kWave) + threadIdx.x / kWave) * kWave;
    if (wave_base >= nq) return;
    const int pos = wave_base + lane;
    const bool valid = pos < nq;
    const float4 q = q_sorted[valid ? pos : nq - 1];
    const bool live = valid && q.x <= FLT_MAX;   // a non-finite query (knn_gather_kernel) searches nothing: its lists stay FLT_MAX, its mean is inf
    float best[K];
#pragma unroll
    for (int k = 0; k < K; ++k) best[k] = FLT_MAX;

    // a first bound from the neighbours along the curve (K on either side); the candidates are looked at again in the box scan
    int centre = pos;
    if (!kSelf) {   // position of the query's code in the reference order
        const uint32_t code = q_codes[valid ? pos : nq - 1];
        int lo = 0, hi = nr;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (r_codes[mid] < code) lo = mid + 1; else hi = mid; }
        centre = lo;
    }
    for (int o = -K; o <= K; ++o) {
        const int j = centre + o;
        if (j < 0 || j >= nr || (kSelf && o == 0)) continue;
        insert_best<K>(best, dist2(q, r_sorted[j]));
    }
    const float reject = best[K - 1];
#pragma unroll
    for (int k = 0; k < K; ++k) best[k] = FLT_MAX;

    // AABB of the wave's queries
    const float big = FLT_MAX;
    const float wlo[3] = {wave_min(live ? q.x : big), wave_min(live ? q.y : big), wave_min(live ? q.z : big)};
    const float whi[3] = {wave_max(live ? q.x : -big), wave_max(live ? q.y : -big), wave_max(live ? q.z : -big)};
    const float qp[3] = {q.x, q.y, q.z};

    for (int g = 0; g < n_boxes; g += kWave) {
        // the worst bound any lane still has: a box farther than that from the wave's AABB cannot matter to anyone
        const float bound = wave_max(live ? fminf(reject, best[K - 1]) : 0.f);
        bool need = false;
        if (g + lane < n_boxes) need = !(gap2(boxes[2 * (g + lane)], boxes[2 * (g + lane) + 1], wlo, whi) > bound);
        unsigned long long todo = ballot64(need);
        while (todo) {
            const int b = g + __builtin_ctzll(todo);
            todo &= todo - 1;
            // per-lane test as in the published algorithm: skip when the box is farther than this lane's bounds
            const float pd = gap2(boxes[2 * b], boxes[2 * b + 1], qp, qp);
            const bool mine = live && !(pd > reject) && !(pd > best[K - 1]);
            if (ballot64(mine) == 0) continue;
            const int first = b * kKnnBox, last = min(nr, first + kKnnBox);
            for (int j = first; j < last; ++j) {
                const float4 c = r_sorted[j];   // wave-uniform address
                float d = dist2(q, c);
                if (kSelf && j == pos) d = FLT_MAX;
                if (mine) insert_best<K>(best, d);
            }
        }
    }
    if (valid) {
        float sum = best[0];
#pragma unroll
        for (int k = 1; k < K; ++k) sum += best[k];
        const float mean = sum / (float)K;
        out[__float_as_uint(q.w)] = take_sqrt ? sqrtf(mean) : mean;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------
struct KnnLayout {
    size_t partial, bounds, r_codes, r_codes_sorted, r_order, r_sorted, boxes, q_codes, q_codes_sorted, q_order, q_sorted, sort_temp, total;
    int blocks_r, blocks_q, n_boxes;
};

static int bounds_blocks(int n) { const int b = (n + kKnnThreads * 8 - 1) / (kKnnThreads * 8); return b < 1 ? 1 : (b > 1024 ? 1024 : b); }

// ---- the ordering steps, for the search below and for cluster.hip (launch.h) ---------------------------------------------------
size_t cloud_bounds_partial_bytes(int n) { return (size_t)bounds_blocks(n) * 6 * 4; }

hipError_t cloud_bounds_masked(const float* pts, const uint8_t* active, int n, float* partial, float* bounds, hipStream_t s) {
    const int blocks = bounds_blocks(n);
    hipLaunchKernelGGL(knn_bounds_partial_kernel<true>, dim3(blocks), dim3(kKnnThreads), 0, s, pts, active, n, partial);
    hipLaunchKernelGGL(knn_bounds_final_kernel, dim3(1), dim3(64), 0, s, partial, blocks, bounds);
    return hipGetLastError();
}

hipError_t cloud_order(const float* pts, const uint8_t* active, bool masked, int n, const float* bounds, const CloudOrder& o, void* sort_temp,
                       size_t temp_bytes, RankMode rank_mode, hipStream_t s) {
    const dim3 grid((n + 255) / 256), block(256);
    if (masked) hipLaunchKernelGGL(knn_morton_kernel<true>, grid, block, 0, s, pts, active, n, bounds, o.codes);
    else hipLaunchKernelGGL(knn_morton_kernel<false>, grid, block, 0, s, pts, active, n, bounds, o.codes);
    const hipError_t e = radix_sort_pairs(o.codes, nullptr, o.codes_sorted, o.order, (uint32_t)n, masked ? 31 : 30, sort_temp, temp_bytes, s, nullptr,
                                          nullptr, rank_mode, false);
    if (e != hipSuccess) return e;
    if (masked) hipLaunchKernelGGL(knn_gather_kernel<true>, grid, block, 0, s, pts, active, o.order, n, o.sorted);
    else hipLaunchKernelGGL(knn_gather_kernel<false>, grid, block, 0, s, pts, active, o.order, n, o.sorted);
    return hipGetLastError();
}

hipError_t cloud_boxes(const float4* sorted, int n, float4* boxes, hipStream_t s) {
    hipLaunchKernelGGL(knn_boxes_kernel, dim3((n + kKnnBox - 1) / kKnnBox), dim3(kKnnThreads), 0, s, sorted, n, boxes);
    return hipGetLastError();
}

KnnLayout knn_layout(int nq, int nr) {   // nq == 0: self search
    KnnLayout L{};
    Carver c;
    L.blocks_r = bounds_blocks(nr); L.blocks_q = nq > 0 ? bounds_blocks(nq) : 0;
    L.n_boxes = (nr + kKnnBox - 1) / kKnnBox;
    // (the self search has no query regions, an empty cloud no points: such a region takes 256 B all the same)
    const size_t r = nr > 0 ? nr : 1, q = nq > 0 ? nq : 1, boxes = L.n_boxes > 0 ? L.n_boxes : 1;
    L.partial = c.take((size_t)(L.blocks_r + L.blocks_q) * 6 * 4);
    L.bounds = c.take(6 * 4);
    L.r_codes = c.take(r * 4); L.r_codes_sorted = c.take(r * 4); L.r_order = c.take(r * 4);
    L.r_sorted = c.take(r * 16);
    L.boxes = c.take(boxes * 32);
    L.q_codes = c.take(q * 4); L.q_codes_sorted = c.take(q * 4); L.q_order = c.take(q * 4);
    L.q_sorted = c.take(q * 16);
    L.sort_temp = c.take(radix_sort_temp_bytes((uint32_t)(nq > nr ? nq : nr)));
    L.total = c.off;
    return L;
}

static size_t knn_workspace_bytes(int nq, int nr) { return knn_layout(nq, nr).total; }

// query == nullptr / nq == 0: every reference point against the others
static hipError_t knn_mean_dist2(int nq, const float* query, int nr, const float* reference, int K, int take_sqrt, float* out, void* ws,
                          size_t ws_bytes, RankMode rank_mode, hipStream_t s) {
    const bool self = query == nullptr;
    if (self) nq = 0;
    const KnnLayout L = knn_layout(nq, nr);
    if (ws_bytes < L.total) return hipErrorInvalidValue;
    float* partial = at<float>(ws, L.partial); float* bounds = at<float>(ws, L.bounds);
    const uint8_t* const all = nullptr;   // the kNN's clouds carry no mask
    hipLaunchKernelGGL(knn_bounds_partial_kernel<false>, dim3(L.blocks_r), dim3(kKnnThreads), 0, s, reference, all, nr, partial);
    if (!self) hipLaunchKernelGGL(knn_bounds_partial_kernel<false>, dim3(L.blocks_q), dim3(kKnnThreads), 0, s, query, all, nq, partial + 6 * L.blocks_r);
    hipLaunchKernelGGL(knn_bounds_final_kernel, dim3(1), dim3(64), 0, s, partial, L.blocks_r + L.blocks_q, bounds);
    const size_t temp_bytes = radix_sort_temp_bytes((uint32_t)(nq > nr ? nq : nr));
    auto order = [&](const float* pts, int n, size_t codes, size_t codes_sorted, size_t order, size_t sorted) {
        const CloudOrder o{at<uint32_t>(ws, codes), at<uint32_t>(ws, codes_sorted), at<uint32_t>(ws, order), at<float4>(ws, sorted)};
        return cloud_order(pts, all, false, n, bounds, o, at<void>(ws, L.sort_temp), temp_bytes, rank_mode, s);
    };
    hipError_t e = order(reference, nr, L.r_codes, L.r_codes_sorted, L.r_order, L.r_sorted);
    if (e != hipSuccess) return e;
    e = cloud_boxes(at<float4>(ws, L.r_sorted), nr, at<float4>(ws, L.boxes), s);
    if (e != hipSuccess) return e;
    if (!self) {
        e = order(query, nq, L.q_codes, L.q_codes_sorted, L.q_order, L.q_sorted);
        if (e != hipSuccess) return e;
    }
    const int n_search = self ? nr : nq;
    const dim3 grid((n_search + kKnnThreads - 1) / kKnnThreads), block(kKnnThreads);
    const float4* rs = at<float4>(ws, L.r_sorted);
    const float4* qs = self ? rs : at<float4>(ws, L.q_sorted);
    const uint32_t* rc = at<uint32_t>(ws, L.r_codes_sorted);
    const uint32_t* qc = self ? rc : at<uint32_t>(ws, L.q_codes_sorted);
    const float4* boxes = at<float4>(ws, L.boxes);
#define SR_KNN_LAUNCH(KK, SELF) \
    hipLaunchKernelGGL((knn_search_kernel<KK, SELF>), grid, block, 0, s, qs, n_search, rs, rc, qc, nr, boxes, L.n_boxes, take_sqrt, out)
    if (K == 3) { if (self) SR_KNN_LAUNCH(3, true); else SR_KNN_LAUNCH(3, false); }
    else        { if (self) SR_KNN_LAUNCH(10, true); else SR_KNN_LAUNCH(10, false); }
#undef SR_KNN_LAUNCH
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

extern "C" {

size_t sr_knn_workspace_bytes(int32_t n_query, int32_t n_reference) {
    return knn_workspace_bytes(n_query > 0 ? n_query : 0, n_reference > 0 ? n_reference : 0);
}

int sr_knn_mean_dist2(int32_t n_query, const float* query, int32_t n_reference, const float* reference, int32_t K,
                      int32_t take_sqrt, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (K != 3 && K != 10) return fail(SR_ERR_UNSUPPORTED, "K = %d, supported: 3 and 10", K);
    if (n_reference < 0 || (query && n_query < 0)) return fail(SR_ERR_INVALID_ARGUMENT, "negative point count");
    const int nq = query ? n_query : 0;
    if ((query ? nq : n_reference) == 0) return SR_OK;
    if (n_reference == 0) return fail(SR_ERR_INVALID_ARGUMENT, "empty reference cloud");
    if (!reference || !out || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = check_workspace_size(workspace, workspace_bytes, knn_workspace_bytes(nq, n_reference))) return rc;
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), false, &sort_mode)) return rc;
    SR_HIP(knn_mean_dist2(nq, query, n_reference, reference, K, take_sqrt, out, workspace, workspace_bytes, sort_mode, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
