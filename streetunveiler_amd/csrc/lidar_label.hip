// lidar_label.hip -- colouring and labelling the LiDAR returns from the camera frames (include/surfel_raster.h states the semantics)
//   [REF scene/dataset_readers/projection_utils.py:17-104, waymo.py:79-192, kitti.py:117-163, pandaset.py:53-106]
//     lidar_label_decide_kernel<kPerView>   one thread per point, grid row = sweep, the loop over the sweep's cameras inside: projection in
//                                           float64, the in-frame predicate, the four-corner certainty test, the pixel's colour and label.
//                                           One 64-bit row per point (the integer colour sums, the count, the last label) or, kPerView, one
//                                           per (point, camera) at (sweep, camera, point); a flag word per row for the scan
//     exclusive_scan_in_place               (mesh_post.hip) flags -> output rows + the kept count
//     lidar_vote_kernel                     points x ALL views, no certainty test: a thread holds kVoteRows points and their class counts
//                                           (eight 16-bit counters in two 64-bit registers) and walks the views; the first largest class
//     lidar_label_emit_kernel               the kept rows at their scanned offsets: xyz bit for bit, sums / count, label, point index
//     lidar_rows_per_sweep_kernel           the scanned offsets at the sweeps' borders
//
// A sweep is a grid row, so the view index s C + c is the same in every lane of a wave and the 192-byte view record comes through scalar
// loads; the pictures are read where the points land (a gather through L2 / the Infinity Cache: a street's returns of one sweep land in
// runs along the image rows), never staged.  Every index is formed from tested quantities: 0 <= u < w and 0 <= v < h follow from the
// predicate, a corner is read only where its validity test holds, the wrapped fourth column lies in 1 .. w-1 (u + r < w gives u - r > -w),
// sweep borders are clamped to [0, n], an output offset is tested against the row count.  Built with -ffp-contract=off: the projection is
// the float64 operations written below, one rounding each, in this order.
#include <cmath>

#include "abi.h"

namespace sr {

constexpr int kLabelThreads = 256;
constexpr int kVoteRows = 4;                                 // points a thread of lidar_vote_kernel holds
constexpr int kVoteChunk = kVoteRows * kLabelThreads;
constexpr int kLabelMaxCameras = 32;   // a row's colour sums (13 bits each) and its count (6 bits) are sized for it
constexpr int kLabelMaxViews = 65535;  // the vote counts a class in 16 bits; a sweep is a grid row
constexpr int kLabelMaxClasses = 8;
// what a decide / vote and the emit after it share: the cloud, its sweeps (offsets: device [n_sweeps + 1] or nullptr = one sweep of all
// points; max_sweep >= the longest) and how many rows a point has (1, or C in the per-view mode)
struct LabelCloud {
    uint32_t n;
    const void* points;
    int points_f64;
    const int32_t* sweep_offsets;
    int n_sweeps;
    uint32_t max_sweep;
    int rows_per_point;
};

// ---- a row ----------------------------------------------------------------------------------------------------------------------------
// sums of at most 32 bytes: 13 bits each; count 0..32: 6 bits; label: 8 bits
constexpr int kRowG = 13, kRowB = 26, kRowCount = 39, kRowLabel = 45;
__device__ __forceinline__ unsigned long long pack_row(uint32_t r, uint32_t g, uint32_t b, uint32_t count, uint32_t label) {
    return (unsigned long long)r | ((unsigned long long)g << kRowG) | ((unsigned long long)b << kRowB) | ((unsigned long long)count << kRowCount) |
           ((unsigned long long)label << kRowLabel);
}

// ---- the predicate --------------------------------------------------------------------------------------------------------------------
struct LabelPixel {
    bool in;
    int u, v;      // trunc(pix): 0 <= u < w, 0 <= v < h where in
};

__device__ __forceinline__ LabelPixel label_project(const SrLabelView* __restrict__ vw, double x, double y, double z) {
    const double* R = vw->w2c;
    const double* K = vw->K;
    const double cx = ((R[0] * x + R[1] * y) + R[2] * z) + R[3];
    const double cy = ((R[4] * x + R[5] * y) + R[6] * z) + R[7];
    const double cz = ((R[8] * x + R[9] * y) + R[10] * z) + R[11];
    const double px = (K[0] * cx + K[1] * cy) + K[2] * cz;
    const double py = (K[3] * cx + K[4] * cy) + K[5] * cz;
    const double pw = (K[6] * cx + K[7] * cy) + K[8] * cz;
    const double pu = __ddiv_rn(px, pw), pv = __ddiv_rn(py, pw);
    LabelPixel hit;
    // strict, and false for a NaN; 0 < pix < w <= INT32_MAX, so the conversion is exact truncation
    hit.in = pu < (double)vw->w && pu > 0.0 && pv < (double)vw->h && pv > 0.0 && cz > 0.0 && isfinite(x) && isfinite(y) && isfinite(z);
    hit.u = hit.in ? (int)pu : 0;
    hit.v = hit.in ? (int)pv : 0;
    return hit;
}

__device__ __forceinline__ uint32_t label_at(const uint8_t* __restrict__ map, const uint8_t* __restrict__ lut, int w, long long v, long long u) {
    const uint32_t raw = map[(size_t)v * (size_t)w + (size_t)u];
    return lut ? lut[raw] : raw;
}

// no valid corner differs from l0.  A corner is valid as the reference tests it: row v-r > 0 or v+r < h, column u-r > 0 or u+r < w.
__device__ __forceinline__ bool label_certain(const uint8_t* __restrict__ map, const uint8_t* __restrict__ lut, int h, int w, int u, int v, int r,
                                              bool mirrored, uint32_t l0) {
    const long long top = (long long)v - r, bottom = (long long)v + r, left = (long long)u - r, right = (long long)u + r;
    const bool top_ok = top > 0, bottom_ok = bottom < h, left_ok = left > 0, right_ok = right < w;
    bool certain = true;
    if (top_ok && left_ok) certain = certain && label_at(map, lut, w, top, left) == l0;
    if (top_ok && right_ok) certain = certain && label_at(map, lut, w, top, right) == l0;
    if (bottom_ok && left_ok) certain = certain && label_at(map, lut, w, bottom, left) == l0;
    if (bottom_ok && right_ok) {
        // the reference reads column u-r here; negative, it wraps as numpy's index does: -w < u-r follows from u+r < w
        const long long column = mirrored ? right : (left < 0 ? left + w : left);
        certain = certain && label_at(map, lut, w, bottom, column) == l0;
    }
    return certain;
}

__device__ __forceinline__ void load_point(const LabelCloud& c, size_t i, double& x, double& y, double& z) {
    if (c.points_f64) {
        const double* p = static_cast<const double*>(c.points) + 3 * i;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const float* p = static_cast<const float*>(c.points) + 3 * i;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
}

// the points of sweep s, clamped into [0, n] and start <= end whatever the table holds
__device__ __forceinline__ void sweep_range(const LabelCloud& c, int s, uint32_t& start, uint32_t& end) {
    if (!c.sweep_offsets) { start = 0u; end = c.n; return; }
    const int n = (int)c.n;                        // n < 2^31
    const int a = min(max(c.sweep_offsets[s], 0), n);
    const int b = min(max(c.sweep_offsets[s + 1], a), n);
    start = (uint32_t)a;
    end = (uint32_t)b;
}

// ---- decide ---------------------------------------------------------------------------------------------------------------------------
template <bool kPerView>
__global__ __launch_bounds__(kLabelThreads) void lidar_label_decide_kernel(const LabelCloud c, const SrLabelView* __restrict__ views, int C, int check_range,
                                                                           bool mirrored, const uint8_t* __restrict__ lut,
                                                                           unsigned long long* __restrict__ rows, uint32_t* __restrict__ flags) {
    const int s = (int)blockIdx.y;
    uint32_t start, end;
    sweep_range(c, s, start, end);
    const unsigned long long j = (unsigned long long)blockIdx.x * kLabelThreads + threadIdx.x;
    const unsigned long long i = start + j;
    if (i >= end) return;
    const unsigned long long len = end - start;
    double x, y, z;
    load_point(c, (size_t)i, x, y, z);
    uint32_t sr = 0u, sg = 0u, sb = 0u, count = 0u, label = 0u;
    for (int cam = 0; cam < C; ++cam) {
        const SrLabelView* vw = views + ((size_t)s * (size_t)C + (size_t)cam);      // the same in every lane: scalar loads
        const LabelPixel hit = label_project(vw, x, y, z);
        bool take = false;
        uint32_t r = 0u, g = 0u, b = 0u, l0 = 0u;
        if (hit.in) {
            l0 = label_at(vw->map, lut, vw->w, hit.v, hit.u);
            take = label_certain(vw->map, lut, vw->h, vw->w, hit.u, hit.v, check_range, mirrored, l0);
            if (take && vw->image) {
                const uint8_t* px = vw->image + 3 * ((size_t)hit.v * (size_t)vw->w + (size_t)hit.u);
                r = px[0]; g = px[1]; b = px[2];
            }
        }
        if (kPerView) {
            const size_t pos = (size_t)((unsigned long long)start * (unsigned)C + (unsigned long long)cam * len + j);     // < n C < 2^31
            rows[pos] = take ? pack_row(r, g, b, 1u, l0) : 0ull;
            flags[pos] = take ? 1u : 0u;
        } else if (take) {
            sr += r; sg += g; sb += b;
            count += 1u;
            label = l0;                                                             // the last camera wins
        }
    }
    if (!kPerView) {
        rows[i] = pack_row(sr, sg, sb, count, count ? label : 0u);
        flags[i] = count ? 1u : 0u;
    }
}

// ---- the vote -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLabelThreads) void lidar_vote_kernel(const LabelCloud c, const SrLabelView* __restrict__ views, int V, int n_classes,
                                                                   const uint8_t* __restrict__ lut, unsigned long long* __restrict__ rows,
                                                                   uint32_t* __restrict__ flags, uint8_t* __restrict__ valid_mask,
                                                                   unsigned long long* __restrict__ n_bad) {
    double px[kVoteRows], py[kVoteRows], pz[kVoteRows];
    unsigned long long lo[kVoteRows], hi[kVoteRows];         // classes 0..3 and 4..7, 16 bits each: V <= 65535 hits at most
    bool seen[kVoteRows];
    const uint32_t base = blockIdx.x * (uint32_t)kVoteChunk; // n < 2^31 and base < n: base + kVoteChunk does not overflow 32 bits
#pragma unroll
    for (int r = 0; r < kVoteRows; ++r) {
        const uint32_t i = base + (uint32_t)r * kLabelThreads + threadIdx.x;
        px[r] = py[r] = pz[r] = NAN;                         // a NaN is in no view
        if (i < c.n) load_point(c, i, px[r], py[r], pz[r]);
        lo[r] = hi[r] = 0ull;
        seen[r] = false;
    }
    uint32_t bad = 0u;
    for (int f = 0; f < V; ++f) {
        const SrLabelView* vw = views + f;
#pragma unroll
        for (int r = 0; r < kVoteRows; ++r) {
            const LabelPixel hit = label_project(vw, px[r], py[r], pz[r]);
            if (!hit.in) continue;
            const uint32_t label = label_at(vw->map, lut, vw->w, hit.v, hit.u);
            seen[r] = true;
            if (label < (uint32_t)n_classes) {
                const unsigned long long one = 1ull << (16u * (label & 3u));
                if (label < 4u) lo[r] += one; else hi[r] += one;
            } else {
                ++bad;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kVoteRows; ++r) {
        const uint32_t i = base + (uint32_t)r * kLabelThreads + threadIdx.x;
        if (i >= c.n) continue;
        uint32_t best = 0u, tag = 0u;
#pragma unroll
        for (int k = 0; k < kLabelMaxClasses; ++k) {         // strictly greater: the first largest, as argmax
            const uint32_t hits = (uint32_t)((k < 4 ? lo[r] : hi[r]) >> (16 * (k & 3))) & 0xFFFFu;
            if (hits > best) { best = hits; tag = (uint32_t)k; }
        }
        rows[i] = seen[r] ? pack_row(0u, 0u, 0u, 1u, tag) : 0ull;
        flags[i] = seen[r] ? 1u : 0u;
        valid_mask[i] = seen[r] ? 1 : 0;
    }
    if (bad) atomicAdd(n_bad, (unsigned long long)bad);
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLabelThreads) void lidar_label_emit_kernel(const LabelCloud c, const unsigned long long* __restrict__ rows,
                                                                         const uint32_t* __restrict__ offsets, uint32_t n_rows, void* __restrict__ out_xyz,
                                                                         double* __restrict__ out_rgb, int32_t* __restrict__ out_semantics,
                                                                         long long* __restrict__ out_index) {
    const int s = (int)blockIdx.y;
    uint32_t start, end;
    sweep_range(c, s, start, end);
    const unsigned long long j = (unsigned long long)blockIdx.x * kLabelThreads + threadIdx.x;
    const unsigned long long i = start + j;
    if (i >= end) return;
    const unsigned long long len = end - start;
    for (int cam = 0; cam < c.rows_per_point; ++cam) {
        const size_t pos = (size_t)((unsigned long long)start * (unsigned)c.rows_per_point + (unsigned long long)cam * len + j);
        const unsigned long long row = rows[pos];
        const uint32_t count = (uint32_t)(row >> kRowCount) & 63u;
        if (!count) continue;
        const size_t at = offsets[pos];
        if (at >= n_rows) continue;
        if (out_xyz) {                                       // bit for bit, in the input's dtype
            if (c.points_f64) {
                const unsigned long long* src = static_cast<const unsigned long long*>(c.points) + 3 * (size_t)i;
                unsigned long long* dst = static_cast<unsigned long long*>(out_xyz) + 3 * at;
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            } else {
                const uint32_t* src = static_cast<const uint32_t*>(c.points) + 3 * (size_t)i;
                uint32_t* dst = static_cast<uint32_t*>(out_xyz) + 3 * at;
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            }
        }
        if (out_rgb) {                                       // exact integers, one IEEE division
            const double d = (double)count;
            out_rgb[3 * at] = __ddiv_rn((double)((uint32_t)row & 0x1FFFu), d);
            out_rgb[3 * at + 1] = __ddiv_rn((double)((uint32_t)(row >> kRowG) & 0x1FFFu), d);
            out_rgb[3 * at + 2] = __ddiv_rn((double)((uint32_t)(row >> kRowB) & 0x1FFFu), d);
        }
        if (out_semantics) out_semantics[at] = (int32_t)((uint32_t)(row >> kRowLabel) & 0xFFu);
        if (out_index) out_index[at] = (long long)i;
    }
}

__global__ __launch_bounds__(kLabelThreads) void lidar_rows_per_sweep_kernel(const LabelCloud c, const uint32_t* __restrict__ offsets, uint32_t total_rows,
                                                                             uint32_t n_rows, int32_t* __restrict__ rows_per_sweep) {
    const int s = (int)(blockIdx.x * kLabelThreads + threadIdx.x);
    if (s >= c.n_sweeps) return;
    uint32_t start, end;
    sweep_range(c, s, start, end);
    const unsigned long long p0 = (unsigned long long)start * (unsigned)c.rows_per_point, p1 = (unsigned long long)end * (unsigned)c.rows_per_point;
    const uint32_t o0 = p0 >= total_rows ? n_rows : offsets[p0], o1 = p1 >= total_rows ? n_rows : offsets[p1];
    rows_per_sweep[s] = (int32_t)(o1 - o0);
}

// ---- the launchers --------------------------------------------------------------------------------------------------------------------
struct LabelLayout {
    size_t rows, flags, chunks, total;
};
static LabelLayout label_layout(uint64_t rows) {
    LabelLayout L;
    Carver c;
    const size_t r = rows > 0 ? (size_t)rows : 1;
    L.rows = c.take(8 * r);
    L.flags = c.take(4 * r);
    L.chunks = c.take(4 * scan_in_place_chunk_words((uint32_t)r));
    L.total = c.off;
    return L;
}
static size_t lidar_label_workspace_bytes(uint64_t rows) { return label_layout(rows).total; }

static dim3 sweep_grid(const LabelCloud& c) {
    return dim3((unsigned)(((uint64_t)c.max_sweep + kLabelThreads - 1) / kLabelThreads), (unsigned)(c.sweep_offsets ? c.n_sweeps : 1));
}

// c.rows_per_point = 1 (a row a point) or `cameras` (a row per (point, camera)); c.n rows_per_point < 2^31
static hipError_t lidar_label_decide(const LabelCloud& c, const SrLabelView* views, int cameras, int check_range, bool mirrored, const uint8_t* lut, void* ws,
                              uint64_t* counts, hipStream_t s) {
    const uint64_t total = (uint64_t)c.n * (uint64_t)c.rows_per_point;
    const LabelLayout L = label_layout(total);
    unsigned long long* rows = at<unsigned long long>(ws, L.rows);
    uint32_t* flags = at<uint32_t>(ws, L.flags);
    // a row no thread reaches (a sweep table that leaves points out) is an empty row, not stale memory
    hipError_t e = hipMemsetAsync(rows, 0, 8 * (size_t)total, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(flags, 0, 4 * (size_t)total, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    if (c.rows_per_point > 1)      // (with one camera the two modes are the same rows)
        hipLaunchKernelGGL(lidar_label_decide_kernel<true>, sweep_grid(c), dim3(kLabelThreads), 0, s, c, views, cameras, check_range, mirrored, lut, rows, flags);
    else
        hipLaunchKernelGGL(lidar_label_decide_kernel<false>, sweep_grid(c), dim3(kLabelThreads), 0, s, c, views, cameras, check_range, mirrored, lut, rows, flags);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return exclusive_scan_in_place(flags, (uint32_t)total, at<uint32_t>(ws, L.chunks), reinterpret_cast<uint32_t*>(counts), s);   // the low word: little-endian
}

static hipError_t lidar_vote(const LabelCloud& c, const SrLabelView* views, int n_views, int n_classes, const uint8_t* lut, void* ws, uint8_t* valid_mask,
                      uint64_t* counts, hipStream_t s) {
    const LabelLayout L = label_layout(c.n);
    unsigned long long* rows = at<unsigned long long>(ws, L.rows);
    uint32_t* flags = at<uint32_t>(ws, L.flags);
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)(((uint64_t)c.n + kVoteChunk - 1) / kVoteChunk);
    hipLaunchKernelGGL(lidar_vote_kernel, dim3(blocks), dim3(kLabelThreads), 0, s, c, views, n_views, n_classes, lut, rows, flags, valid_mask,
                       reinterpret_cast<unsigned long long*>(counts + 1));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return exclusive_scan_in_place(flags, c.n, at<uint32_t>(ws, L.chunks), reinterpret_cast<uint32_t*>(counts), s);
}

// n_rows >= 1
static hipError_t lidar_label_emit(const LabelCloud& c, const void* ws, uint32_t n_rows, void* out_xyz, double* out_rgb, int32_t* out_semantics, int64_t* out_index,
                            int32_t* rows_per_sweep, hipStream_t s) {
    const uint64_t total = (uint64_t)c.n * (uint64_t)c.rows_per_point;
    const LabelLayout L = label_layout(total);
    const unsigned long long* rows = at<const unsigned long long>(const_cast<void*>(ws), L.rows);
    const uint32_t* offsets = at<const uint32_t>(const_cast<void*>(ws), L.flags);
    if (out_xyz || out_rgb || out_semantics || out_index)
        hipLaunchKernelGGL(lidar_label_emit_kernel, sweep_grid(c), dim3(kLabelThreads), 0, s, c, rows, offsets, n_rows, out_xyz, out_rgb, out_semantics,
                           reinterpret_cast<long long*>(out_index));
    if (rows_per_sweep)
        hipLaunchKernelGGL(lidar_rows_per_sweep_kernel, dim3((unsigned)((c.n_sweeps + kLabelThreads - 1) / kLabelThreads)), dim3(kLabelThreads), 0, s, c, offsets,
                           (uint32_t)total, n_rows, rows_per_sweep);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks the three launching sr_lidar_* calls share: the cloud, the view table and the workspace of n * rows_per_point rows
static int lidar_arguments(int32_t n, const void* points, int32_t points_f64, const void* views, int32_t n_views, const uint8_t* label_lut,
                           int32_t rows_per_point, const void* workspace, size_t workspace_bytes, bool needs_views) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n %d is negative", n);
    if (int rc = check_f32_or_f64("points", nullptr, points_f64)) return rc;   // the flag; the address once there are points
    if (rows_per_point < 1 || rows_per_point > kLabelMaxCameras)
        return fail(SR_ERR_INVALID_ARGUMENT, "%d rows a point: 1..%d", rows_per_point, kLabelMaxCameras);
    if ((uint64_t)n * (uint64_t)rows_per_point >= (1ull << 31))
        return fail(SR_ERR_UNSUPPORTED, "%d points x %d rows: fewer than 2^31 rows a call (fewer sweeps a call)", n, rows_per_point);
    if (needs_views) {
        if (n_views < 1 || n_views > kLabelMaxViews) return fail(SR_ERR_INVALID_ARGUMENT, "n_views = %d: 1..%d", n_views, kLabelMaxViews);
        if (!views) return fail(SR_ERR_INVALID_ARGUMENT, "views is NULL");
        if ((uintptr_t)views & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "views is not 8-B aligned");
        (void)label_lut;       // 256 device bytes or NULL: nothing to check on the host
    }
    if (n == 0) return SR_OK;
    if (!points) return fail(SR_ERR_INVALID_ARGUMENT, "points is NULL");
    if (int rc = check_f32_or_f64("points", points, points_f64)) return rc;
    return check_workspace(workspace, workspace_bytes, lidar_label_workspace_bytes((uint64_t)n * (uint64_t)rows_per_point));
}

static int lidar_sweeps(int32_t n, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points) {
    if (n_sweeps < 1 || n_sweeps > kLabelMaxViews) return fail(SR_ERR_INVALID_ARGUMENT, "n_sweeps = %d: 1..%d", n_sweeps, kLabelMaxViews);
    if ((uintptr_t)sweep_offsets & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "sweep_offsets is not 4-B aligned");
    if (!sweep_offsets && n_sweeps != 1) return fail(SR_ERR_INVALID_ARGUMENT, "sweep_offsets is NULL with %d sweeps", n_sweeps);
    if (max_sweep_points < 0 || max_sweep_points > n) return fail(SR_ERR_INVALID_ARGUMENT, "max_sweep_points = %d: not in 0..n = %d", max_sweep_points, n);
    if (n > 0 && max_sweep_points < 1) return fail(SR_ERR_INVALID_ARGUMENT, "max_sweep_points = 0 with %d points", n);
    return SR_OK;
}

extern "C" {

size_t sr_lidar_label_workspace_bytes(int32_t n, int32_t rows_per_point) {
    if (n < 0 || rows_per_point < 1 || rows_per_point > kLabelMaxCameras || (uint64_t)n * (uint64_t)rows_per_point >= (1ull << 31)) return 0;
    return lidar_label_workspace_bytes((uint64_t)n * (uint64_t)rows_per_point);
}

int sr_lidar_label_decide(int32_t n, const void* points, int32_t points_f64, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points,
                          const void* views, int32_t n_views, int32_t cameras_per_sweep, int32_t check_range, int32_t fourth_corner,
                          const uint8_t* label_lut, int32_t per_view, void* workspace, size_t workspace_bytes, uint64_t* counts, void* stream) {
    if (cameras_per_sweep < 1 || cameras_per_sweep > kLabelMaxCameras)
        return fail(SR_ERR_INVALID_ARGUMENT, "cameras_per_sweep = %d: 1..%d", cameras_per_sweep, kLabelMaxCameras);
    if (per_view != 0 && per_view != 1) return fail(SR_ERR_INVALID_ARGUMENT, "per_view = %d: 0 or 1", per_view);
    const int32_t rows_per_point = per_view ? cameras_per_sweep : 1;
    if (int rc = lidar_arguments(n, points, points_f64, views, n_views, label_lut, rows_per_point, workspace, workspace_bytes, true)) return rc;
    if (int rc = lidar_sweeps(n, sweep_offsets, n_sweeps, max_sweep_points)) return rc;
    if ((int64_t)n_sweeps * cameras_per_sweep > n_views)
        return fail(SR_ERR_INVALID_ARGUMENT, "%d sweeps x %d cameras > %d views", n_sweeps, cameras_per_sweep, n_views);
    if (check_range < 0) return fail(SR_ERR_INVALID_ARGUMENT, "check_range %d is negative", check_range);
    if (fourth_corner != 0 && fourth_corner != 1) return fail(SR_ERR_INVALID_ARGUMENT, "fourth_corner = %d: 0 (the reference's column) or 1 (mirrored)", fourth_corner);
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if ((uintptr_t)counts & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "counts is not 8-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) { SR_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s)); return SR_OK; }
    const LabelCloud c{(uint32_t)n, points, points_f64, sweep_offsets, n_sweeps, (uint32_t)max_sweep_points, rows_per_point};
    SR_HIP(lidar_label_decide(c, static_cast<const SrLabelView*>(views), cameras_per_sweep, check_range, fourth_corner == 1, label_lut, workspace, counts, s));
    return SR_OK;
}

int sr_lidar_label_emit(int32_t n, const void* points, int32_t points_f64, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points,
                        int32_t rows_per_point, void* workspace, size_t workspace_bytes, int32_t n_rows, void* out_xyz, double* out_rgb,
                        int32_t* out_semantics, int64_t* out_index, int32_t* rows_per_sweep, void* stream) {
    if (int rc = lidar_arguments(n, points, points_f64, nullptr, 0, nullptr, rows_per_point, workspace, workspace_bytes, false)) return rc;
    if (int rc = lidar_sweeps(n, sweep_offsets, n_sweeps, max_sweep_points)) return rc;
    if (n_rows < 0 || (int64_t)n_rows > (int64_t)n * rows_per_point)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_rows = %d: not in 0..%lld", n_rows, (long long)n * rows_per_point);
    if ((uintptr_t)out_xyz & (points_f64 ? 7u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "out_xyz is not aligned to the points' element size");
    if (((uintptr_t)out_rgb | (uintptr_t)out_index) & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "out_rgb or out_index is not 8-B aligned");
    if (((uintptr_t)out_semantics | (uintptr_t)rows_per_sweep) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "out_semantics or rows_per_sweep is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {
        if (rows_per_sweep) SR_HIP(hipMemsetAsync(rows_per_sweep, 0, sizeof(int32_t) * (size_t)n_sweeps, s));
        return SR_OK;
    }
    const LabelCloud c{(uint32_t)n, points, points_f64, sweep_offsets, n_sweeps, (uint32_t)max_sweep_points, rows_per_point};
    SR_HIP(lidar_label_emit(c, workspace, (uint32_t)n_rows, out_xyz, out_rgb, out_semantics, out_index, rows_per_sweep, s));
    return SR_OK;
}

int sr_lidar_vote(int32_t n, const void* points, int32_t points_f64, const void* views, int32_t n_views, int32_t n_classes, const uint8_t* label_lut,
                  void* workspace, size_t workspace_bytes, uint8_t* valid_mask, uint64_t* counts, void* stream) {
    if (int rc = lidar_arguments(n, points, points_f64, views, n_views, label_lut, 1, workspace, workspace_bytes, true)) return rc;
    if (n_classes < 1 || n_classes > kLabelMaxClasses) return fail(SR_ERR_INVALID_ARGUMENT, "n_classes = %d: 1..%d", n_classes, kLabelMaxClasses);
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if ((uintptr_t)counts & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "counts is not 8-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) { SR_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s)); return SR_OK; }
    if (!valid_mask) return fail(SR_ERR_INVALID_ARGUMENT, "valid_mask is NULL");
    const LabelCloud c{(uint32_t)n, points, points_f64, nullptr, 1, (uint32_t)n, 1};
    SR_HIP(lidar_vote(c, static_cast<const SrLabelView*>(views), n_views, n_classes, label_lut, workspace, valid_mask, counts, s));
    return SR_OK;
}

}  // extern "C"
