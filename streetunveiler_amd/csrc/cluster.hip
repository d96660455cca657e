// Radius clustering of a point cloud == what GaussianModel.cluster_instance_with_mask / cluster_semantic_instance compute with
// parallel=False [REF /root/reference/scene/gaussian_model.py:579-651]: the connected components of the graph "two active points are
// joined when sqrtf((dx*dx + dy*dy) + dz*dz) < threshold", each named by its smallest point index.
//
// The search is the kNN's with a constant bound (knn.hip: Morton order, boxes of 512 curve-consecutive points, one wave64 per 64
// consecutive queries, wave-uniform candidates), and every edge is looked at once: a query scans the candidates BEFORE its own place on
// the curve.  On top of it sits the lock-free union-find of union_find.h over the ORIGINAL point indices: a root is only ever hooked under
// a SMALLER root, so the root of a finished tree is the smallest index of its component and the labels do not depend on the order in
// which the unions raced; no lane waits for another.
// Integer / latency / VALU work only; no LDS, no MFMA.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "cloud.h"
#include "abi.h"
#include "union_find.h"

namespace sr {

constexpr int kClusterThreads = 256;

__global__ __launch_bounds__(kClusterThreads) void cluster_init_kernel(int n, int* __restrict__ parent) {
    const long long i = (long long)blockIdx.x * kClusterThreads + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

// One wave = 64 curve-consecutive queries.  sorted[] holds the points that take part first, in Morton order, and every other point behind
// them as (inf, inf, inf) (knn.hip, masked ordering); `d2_below` is the predicate as a bound on the squared distance (cluster_d2_below).
__global__ __launch_bounds__(kClusterThreads) void cluster_edges_kernel(const float4* __restrict__ sorted, int n, const float4* __restrict__ boxes,
                                                                         float d2_below, int* parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long wave_base = ((long long)blockIdx.x * (kClusterThreads / kWave) + threadIdx.x / kWave) * kWave;
    if (wave_base >= n) return;
    const bool valid = wave_base + lane < n;
    const int pos = valid ? (int)(wave_base + lane) : n - 1;
    const float4 q = sorted[pos];
    const bool live = valid && q.x <= FLT_MAX;
    if (ballot64(live) == 0) return;   // the tail of the curve: nobody here takes part
    const int qi = __float_as_int(q.w);

    const float big = FLT_MAX;
    const float wlo[3] = {wave_min(live ? q.x : big), wave_min(live ? q.y : big), wave_min(live ? q.z : big)};
    const float whi[3] = {wave_max(live ? q.x : -big), wave_max(live ? q.y : -big), wave_max(live ? q.z : -big)};
    const float qp[3] = {q.x, q.y, q.z};

    const int own_box = (int)(wave_base / kKnnBox);   // 64 divides 512: the wave's queries share a box
    const int limit = (int)(wave_base + kWave - 1 < n ? wave_base + kWave - 1 : n);   // candidates end before the wave's last query
    for (int g = 0; g <= own_box; g += kWave) {
        bool need = false;
        if (g + lane <= own_box) need = gap2(boxes[2 * (size_t)(g + lane)], boxes[2 * (size_t)(g + lane) + 1], wlo, whi) < d2_below;
        unsigned long long todo = ballot64(need);
        while (todo) {
            const int b = g + __builtin_ctzll(todo);
            todo &= todo - 1;
            const bool mine = live && gap2(boxes[2 * (size_t)b], boxes[2 * (size_t)b + 1], qp, qp) < d2_below;
            if (ballot64(mine) == 0) continue;
            const int first = b * kKnnBox, last = first + min(kKnnBox, limit - first);
            for (int j = first; j < last; ++j) {
                const float4 c = sorted[j];   // wave-uniform address
                const bool hit = mine && j < pos && dist2(q, c) < d2_below;
                if (hit) {
                    const int ci = __float_as_int(c.w);
                    // in a dense cluster almost every edge joins what is joined already: two loads, no atomic
                    if (load_parent(parent, qi) != load_parent(parent, ci)) unite(parent, qi, ci);
                }
            }
        }
    }
}

// After the edge kernel has finished (the kernel boundary is the fence): labels by ORIGINAL index, read off the sorted array, which knows
// who took part.
__global__ __launch_bounds__(kClusterThreads) void cluster_labels_kernel(const float4* __restrict__ sorted, const uint8_t* __restrict__ active, int n,
                                                                          int* parent, long long* __restrict__ labels) {
    const long long pos = (long long)blockIdx.x * kClusterThreads + threadIdx.x;
    if (pos >= n) return;
    const float4 p = sorted[pos];
    const int i = __float_as_int(p.w);
    if (p.x <= FLT_MAX) labels[i] = find_root(parent, i);
    else labels[i] = (active && !active[i]) ? -1 : i;   // masked out | active with a NaN / inf coordinate: in range of nobody, itself included
}

struct ClusterLayout {
    size_t partial, bounds, codes, codes_sorted, order, sorted, boxes, parent, sort_temp, total;
    int n_boxes;
};

static ClusterLayout cluster_layout(int n) {
    ClusterLayout L{};
    Carver c;
    L.n_boxes = (int)(((long long)n + kKnnBox - 1) / kKnnBox);
    const size_t points = n > 0 ? n : 1, boxes = L.n_boxes > 0 ? L.n_boxes : 1;   // (an empty cloud's regions take 256 B each all the same)
    L.partial = c.take(cloud_bounds_partial_bytes(n));
    L.bounds = c.take(6 * 4);
    L.codes = c.take(points * 4); L.codes_sorted = c.take(points * 4); L.order = c.take(points * 4);
    L.sorted = c.take(points * 16);
    L.boxes = c.take(boxes * 32);
    L.parent = c.take(points * 4);
    L.sort_temp = c.take(radix_sort_temp_bytes((uint32_t)n));
    L.total = c.off;
    return L;
}

// sqrtf(d2) < r  <=>  d2 < T, with T the smallest float32 whose root is not below r: sqrtf is correctly rounded, hence monotone, so the
// float32 values split into those below T, whose root is below r, and the rest.  r * r lies within a few steps of T; the two loops walk
// there whichever side it is on.  (r == 0: T = 0, no pair.  A root is taken nowhere else: the kernels compare squared distances with T.)
static float cluster_d2_below(float r) {
    float t = r * r;
    while (t > 0.f && sqrtf(nextafterf(t, -INFINITY)) >= r) t = nextafterf(t, -INFINITY);
    while (sqrtf(t) < r) t = nextafterf(t, INFINITY);
    return t;
}

static size_t cluster_workspace_bytes(int n) { return cluster_layout(n).total; }

// n >= 1; radius finite and >= 0
static hipError_t cluster_radius(int n, const float* xyz, const uint8_t* active, float radius, int64_t* labels, void* ws, size_t ws_bytes,
                          RankMode rank_mode, hipStream_t s) {
    const ClusterLayout L = cluster_layout(n);
    if (ws_bytes < L.total) return hipErrorInvalidValue;
    float* bounds = at<float>(ws, L.bounds);
    const CloudOrder o{at<uint32_t>(ws, L.codes), at<uint32_t>(ws, L.codes_sorted), at<uint32_t>(ws, L.order), at<float4>(ws, L.sorted)};
    int* parent = at<int>(ws, L.parent);
    const dim3 grid((unsigned)(((long long)n + kClusterThreads - 1) / kClusterThreads)), block(kClusterThreads);
    hipError_t e = cloud_bounds_masked(xyz, active, n, at<float>(ws, L.partial), bounds, s);
    if (e != hipSuccess) return e;
    e = cloud_order(xyz, active, true, n, bounds, o, at<void>(ws, L.sort_temp), radix_sort_temp_bytes((uint32_t)n), rank_mode, s);
    if (e != hipSuccess) return e;
    e = cloud_boxes(o.sorted, n, at<float4>(ws, L.boxes), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cluster_init_kernel, grid, block, 0, s, n, parent);
    hipLaunchKernelGGL(cluster_edges_kernel, grid, block, 0, s, o.sorted, n, at<float4>(ws, L.boxes), cluster_d2_below(radius), parent);
    hipLaunchKernelGGL(cluster_labels_kernel, grid, block, 0, s, o.sorted, active, n, parent, reinterpret_cast<long long*>(labels));
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

extern "C" {

size_t sr_cluster_workspace_bytes(int32_t n) { return cluster_workspace_bytes(n > 0 ? n : 0); }

int sr_cluster_radius(int32_t n, const float* xyz, const uint8_t* active, float radius, int64_t* labels, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "negative point count");
    if (!(radius >= 0.f && radius <= FLT_MAX)) return fail(SR_ERR_INVALID_ARGUMENT, "radius %g is not a finite number >= 0", (double)radius);
    if (n == 0) return SR_OK;
    if (!xyz || !labels || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = check_workspace_size(workspace, workspace_bytes, cluster_workspace_bytes(n))) return rc;
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), false, &sort_mode)) return rc;
    SR_HIP(cluster_radius(n, xyz, active, radius, labels, workspace, workspace_bytes, sort_mode, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
