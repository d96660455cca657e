// voxel.hip -- the semantic voxel downsample a street scene starts from (include/surfel_raster.h states the semantics)
// [REF utils/pcd_utils.py:73-142]: tens of millions of LiDAR returns -> one point per occupied voxel (the means of its members' positions,
// colours and normals, its most frequent label) with the voxels dropped whose label is not 80 % pure.
//   voxel_bounds_kernel / voxel_bounds_finalize_kernel   min and max of the finite rows (order-free) + the number of non-finite rows
//   voxel_key_kernel<T>        the 64-bit voxel index of every point, in the points' own dtype: c = trunc((p - lo) / v), ONE IEEE
//                              subtraction and ONE IEEE division per axis, index = c.x + offset c.y + offset^2 c.z; the sort words
//                              (label in the lowest digit), the label byte, the count of labels outside 0..255
//   radix_sort_pairs           (radix_sort.hip, unchanged) in chained 32-bit passes over the sort words, the value carrying the permutation;
//                              voxel_gather_words_kernel brings the next word into the order the last pass left
//   voxel_sorted_kernel        the index and the label of every point in sorted order;  voxel_heads_kernel: a neighbour compare
//   exclusive_scan_in_place    (mesh_post.hip) heads -> voxel ids + the voxel count
//   voxel_starts_kernel        the first member of every voxel
//   voxel_stats_kernel         per voxel: member count, longest label run (the runs are contiguous: the label is the lowest sort digit),
//                              the keep flag 5 max >= 4 n in integers.  A voxel of more than kVoxelHeavy members is not walked by one lane:
//                              it is queued (an integer atomic) and voxel_stats_heavy_kernel gives it a wave and a 256-bin LDS histogram
//   exclusive_scan_in_place    keep flags -> output rows + the kept count
//   voxel_emit_kernel / voxel_emit_heavy_kernel   the means and labels of the kept voxels, in ascending voxel index
// Sums are float64, the members added in sorted order (label, then input index: the sort is stable) by one lane, or -- a heavy voxel --
// lane l adding members l, l + 64, ... and a butterfly over the lanes: the order of every addition depends on the inputs alone.  The mean is
// sum / count in float64, rounded once to float32.  Integer atomics only (the bad-label counter, the heavy queue's cursor, the LDS
// histogram); the queue's ORDER varies from run to run, what is computed per queued voxel does not.
// Every index is tested before it is used: a permutation entry and a member range against n, a voxel id against the voxel count on the
// device, an output row against the rows the caller allocated, a queue slot against the queue's capacity.
// Built with -ffp-contract=off: the voxel coordinate is a bit-exact contract.
#include <cfloat>
#include <cmath>

#include "abi.h"
#include "scan.h"

namespace sr {

constexpr int kVoxelThreads = 256;
constexpr int kVoxelBoundRows = 8;                                   // points a thread of the bounds kernel takes
constexpr int kVoxelBoundChunk = kVoxelBoundRows * kVoxelThreads;    // 2048 points a block
constexpr int kVoxelHeavyBlocks = 1024;                              // blocks of four waves that drain the heavy queue
constexpr int kVoxelHeavy = 128;                                     // a voxel of more members than this gets a wave instead of a lane
constexpr long long kVoxelMaxOffset = 1ll << 21;                     // offset^3 must stay inside int64

// ---- loads ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double load_real(const void* __restrict__ p, int is_f64, size_t i) {
    return is_f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];   // (float -> double is exact)
}

// ---- bounds -----------------------------------------------------------------------------------------------------------------------------
// partials[7 b + {0..2}] = min, {3..5} = max over the finite rows of block b (+inf / -inf where it has none), [6] = its non-finite rows
__device__ __forceinline__ void voxel_fold_bounds(double (&v)[7], double* red) {
    // red: 7 * kVoxelThreads doubles; min / max / sum are exact and order-free (the count is an integer below 2^31)
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k) red[k * kVoxelThreads + t] = v[k];
    __syncthreads();
    for (int s = kVoxelThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k * kVoxelThreads + t] = fmin(red[k * kVoxelThreads + t], red[k * kVoxelThreads + t + s]);
#pragma unroll
            for (int k = 3; k < 6; ++k) red[k * kVoxelThreads + t] = fmax(red[k * kVoxelThreads + t], red[k * kVoxelThreads + t + s]);
            red[6 * kVoxelThreads + t] += red[6 * kVoxelThreads + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = red[k * kVoxelThreads];
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_bounds_kernel(uint32_t n, const void* __restrict__ pts, int is_f64, double* __restrict__ partials) {
    __shared__ double red[7 * kVoxelThreads];
    double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    const uint32_t base = blockIdx.x * (uint32_t)kVoxelBoundChunk;   // n < 2^31 and base < n: base + 2047 does not overflow
    for (int r = 0; r < kVoxelBoundRows; ++r) {
        const uint32_t i = base + (uint32_t)r * kVoxelThreads + threadIdx.x;
        if (i >= n) continue;
        const double x = load_real(pts, is_f64, 3 * (size_t)i), y = load_real(pts, is_f64, 3 * (size_t)i + 1), z = load_real(pts, is_f64, 3 * (size_t)i + 2);
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            v[0] = fmin(v[0], x); v[1] = fmin(v[1], y); v[2] = fmin(v[2], z);
            v[3] = fmax(v[3], x); v[4] = fmax(v[4], y); v[5] = fmax(v[5], z);
        } else {
            v[6] += 1.0;
        }
    }
    voxel_fold_bounds(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) partials[7 * (size_t)blockIdx.x + k] = v[k];
    }
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_bounds_finalize_kernel(const double* __restrict__ partials, int n_blocks, double* __restrict__ bounds) {
    __shared__ double red[7 * kVoxelThreads];
    double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    for (int b = threadIdx.x; b < n_blocks; b += kVoxelThreads) {
        const double* p = partials + 7 * (size_t)b;
        v[0] = fmin(v[0], p[0]); v[1] = fmin(v[1], p[1]); v[2] = fmin(v[2], p[2]);
        v[3] = fmax(v[3], p[3]); v[4] = fmax(v[4], p[4]); v[5] = fmax(v[5], p[5]);
        v[6] += p[6];
    }
    voxel_fold_bounds(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) bounds[k] = v[k];
    }
}

// ---- keys -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float voxel_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double voxel_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float voxel_trunc(float a) { return truncf(a); }
__device__ __forceinline__ double voxel_trunc(double a) { return trunc(a); }

struct VoxelFrame {        // a kernel parameter, by value: lo and voxel_size are values of the points' dtype, held exactly in doubles
    double lo[3], voxel_size;
    long long offset;
    int label_bits;        // 8 with semantics, 0 without
    int label_bytes;       // 4 or 8: the width of a (signed) label
};

// the coordinate as an integer; a finite point of a cloud whose bounds gave lo and offset lies in [0, offset) -- anything else (the caller
// handed other points than it took the bounds of) is clamped there, so that an index never leaves [0, offset^3)
template <class T>
__device__ __forceinline__ long long voxel_coord(T p, T lo, T v, long long offset) {
    const T c = voxel_trunc(voxel_div(p - lo, v));
    if (!(c >= (T)0)) return 0;                      // (also a NaN)
    if (c >= (T)offset) return offset - 1;
    return (long long)c;
}

template <class T>
__global__ __launch_bounds__(kVoxelThreads) void voxel_key_kernel(uint32_t n, const T* __restrict__ pts, const void* __restrict__ labels, VoxelFrame f,
                                                                  long long* __restrict__ index, uint8_t* __restrict__ label8, uint32_t* __restrict__ w0,
                                                                  uint32_t* __restrict__ w1, uint32_t* __restrict__ w2, uint32_t* __restrict__ n_bad) {
    const uint32_t i = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (i >= n) return;
    const T v = (T)f.voxel_size;
    const long long cx = voxel_coord<T>(pts[3 * (size_t)i], (T)f.lo[0], v, f.offset);
    const long long cy = voxel_coord<T>(pts[3 * (size_t)i + 1], (T)f.lo[1], v, f.offset);
    const long long cz = voxel_coord<T>(pts[3 * (size_t)i + 2], (T)f.lo[2], v, f.offset);
    const long long idx = cx + f.offset * cy + f.offset * f.offset * cz;      // < offset^3 <= 2^63
    uint32_t lab = 0u;
    if (labels) {
        const long long l = f.label_bytes == 8 ? static_cast<const long long*>(labels)[i] : (long long)static_cast<const int32_t*>(labels)[i];
        if (l < 0 || l > 255) atomicAdd(n_bad, 1u);
        lab = (uint32_t)(l & 255);
    }
    index[i] = idx;
    label8[i] = (uint8_t)lab;
    const unsigned long long u = (unsigned long long)idx;
    if (f.label_bits) {
        w0[i] = (uint32_t)(u << 8) | lab;
        w1[i] = (uint32_t)(u >> 24);
        w2[i] = (uint32_t)(u >> 56);
    } else {
        w0[i] = (uint32_t)u;
        w1[i] = (uint32_t)(u >> 32);
        w2[i] = 0u;
    }
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_gather_words_kernel(uint32_t n, const uint32_t* __restrict__ words, const uint32_t* __restrict__ perm,
                                                                           uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    out[i] = j < n ? words[j] : 0u;
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_sorted_kernel(uint32_t n, const long long* __restrict__ index, const uint8_t* __restrict__ label8,
                                                                     const uint32_t* __restrict__ perm, long long* __restrict__ sorted_index,
                                                                     uint8_t* __restrict__ sorted_label) {
    const uint32_t i = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    sorted_index[i] = j < n ? index[j] : 0;
    sorted_label[i] = j < n ? label8[j] : 0;
}

__device__ __forceinline__ bool voxel_is_head(const long long* __restrict__ sorted_index, uint32_t i) {
    return i == 0u || sorted_index[i] != sorted_index[i - 1];
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_heads_kernel(uint32_t n, const long long* __restrict__ sorted_index, uint32_t* __restrict__ heads) {
    const uint32_t i = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (i < n) heads[i] = voxel_is_head(sorted_index, i) ? 1u : 0u;
}

// voxel_id: the exclusive scan of the heads; start[v] = the first sorted position of voxel v
__global__ __launch_bounds__(kVoxelThreads) void voxel_starts_kernel(uint32_t n, const long long* __restrict__ sorted_index, const uint32_t* __restrict__ voxel_id,
                                                                     uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (i >= n || !voxel_is_head(sorted_index, i)) return;
    const uint32_t v = voxel_id[i];
    if (v < n) start[v] = i;
}

// ---- per voxel --------------------------------------------------------------------------------------------------------------------------
// meta: {voxels, kept, bad labels, heavy voxels} on the device
struct VoxelRange { uint32_t begin, end; };
__device__ __forceinline__ VoxelRange voxel_range(const uint32_t* __restrict__ start, uint32_t v, uint32_t nv, uint32_t n) {
    uint32_t b = start[v], e = v + 1u < nv ? start[v + 1u] : n;
    if (e > n) e = n;
    if (b > e) b = e;
    return VoxelRange{b, e};
}
__device__ __forceinline__ uint32_t voxel_keep(uint32_t longest, uint32_t members) {
    return 5ull * (unsigned long long)longest >= 4ull * (unsigned long long)members ? 1u : 0u;
}

// one lane per voxel; thread v >= voxels clears its keep flag (the scan that follows runs over n words).  vlabel[v]: the label, -1 = dropped
__global__ __launch_bounds__(kVoxelThreads) void voxel_stats_kernel(uint32_t n, int has_labels, int heavy_from, const uint32_t* __restrict__ start,
                                                                    const uint8_t* __restrict__ sorted_label, uint32_t* __restrict__ meta,
                                                                    uint32_t* __restrict__ keep, int32_t* __restrict__ vlabel,
                                                                    uint32_t* __restrict__ heavy, uint32_t heavy_capacity) {
    const uint32_t v = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    if (v >= n) return;
    const uint32_t nv = meta[0] < n ? meta[0] : n;
    if (v >= nv) { keep[v] = 0u; vlabel[v] = -1; return; }
    const VoxelRange r = voxel_range(start, v, nv, n);
    const uint32_t members = r.end - r.begin;
    if (members > (uint32_t)heavy_from) {
        const uint32_t slot = atomicAdd(meta + 3, 1u);
        if (slot < heavy_capacity) heavy[slot] = v;
        if (has_labels) return;          // voxel_stats_heavy_kernel decides
    }
    if (!has_labels) { keep[v] = members > 0u ? 1u : 0u; vlabel[v] = members > 0u ? 0 : -1; return; }
    uint32_t longest = 0u, best = 0u, run = 0u, cur = 0u;
    for (uint32_t i = r.begin; i < r.end; ++i) {
        const uint32_t l = sorted_label[i];
        run = (i > r.begin && l == cur) ? run + 1u : 1u;
        cur = l;
        if (run > longest) { longest = run; best = l; }      // the first of equally long runs: the lowest label
    }
    const uint32_t k = members > 0u ? voxel_keep(longest, members) : 0u;
    keep[v] = k;
    vlabel[v] = k ? (int32_t)best : -1;
}

// a wave per queued voxel: the labels counted in 256 LDS bins, the largest bin (the lowest label of equally large ones)
__global__ __launch_bounds__(kVoxelThreads) void voxel_stats_heavy_kernel(uint32_t n, const uint32_t* __restrict__ start, const uint8_t* __restrict__ sorted_label,
                                                                          const uint32_t* __restrict__ meta, uint32_t* __restrict__ keep,
                                                                          int32_t* __restrict__ vlabel, const uint32_t* __restrict__ heavy,
                                                                          uint32_t heavy_capacity) {
    __shared__ uint32_t bins[kVoxelThreads / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t nv = meta[0] < n ? meta[0] : n;
    const uint32_t n_heavy = meta[3] < heavy_capacity ? meta[3] : heavy_capacity;
    const uint32_t n_waves = gridDim.x * (uint32_t)(kVoxelThreads / 64);
    for (uint32_t h = blockIdx.x * (uint32_t)(kVoxelThreads / 64) + (uint32_t)w; h < n_heavy; h += n_waves) {   // (wave-uniform)
        const uint32_t v = heavy[h];
        if (v >= nv) continue;
        const VoxelRange r = voxel_range(start, v, nv, n);
        for (int b = lane; b < 256; b += 64) bins[w][b] = 0u;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = r.begin + (uint32_t)lane; i < r.end; i += 64u) atomicAdd(&bins[w][sorted_label[i]], 1u);
        __builtin_amdgcn_wave_barrier();
        uint32_t longest = 0u, best = 0u;
        for (int b = lane; b < 256; b += 64) {               // ascending labels: > keeps the lowest
            const uint32_t c = bins[w][b];
            if (c > longest) { longest = c; best = (uint32_t)b; }
        }
        for (int m = 32; m > 0; m >>= 1) {
            const uint32_t oc = __shfl_xor(longest, m), ob = __shfl_xor(best, m);
            if (oc > longest || (oc == longest && ob < best)) { longest = oc; best = ob; }
        }
        __builtin_amdgcn_wave_barrier();                     // the bins are read before the next voxel clears them
        if (lane == 0) {
            const uint32_t members = r.end - r.begin;
            const uint32_t k = members > 0u ? voxel_keep(longest, members) : 0u;
            keep[v] = k;
            vlabel[v] = k ? (int32_t)best : -1;
        }
    }
}

struct VoxelEmit {         // a kernel parameter, by value: device pointers; a NULL attribute or output is skipped
    uint32_t n, rows;      // points; rows the caller allocated (the kept count it read back)
    int heavy_from;
    const void *points, *colors, *normals;
    int points_f64, colors_f64, normals_f64;
    const uint32_t *perm, *start, *row, *meta;
    const int32_t* vlabel;
    const long long* sorted_index;
    float *out_points, *out_colors, *out_normals;
    int32_t *out_labels, *out_counts;
    long long* out_index;
};

__device__ __forceinline__ void voxel_add_member(const VoxelEmit& a, uint32_t j, double (&s)[9]) {
    const size_t b = 3 * (size_t)j;
    s[0] += load_real(a.points, a.points_f64, b); s[1] += load_real(a.points, a.points_f64, b + 1); s[2] += load_real(a.points, a.points_f64, b + 2);
    if (a.colors) { s[3] += load_real(a.colors, a.colors_f64, b); s[4] += load_real(a.colors, a.colors_f64, b + 1); s[5] += load_real(a.colors, a.colors_f64, b + 2); }
    if (a.normals) { s[6] += load_real(a.normals, a.normals_f64, b); s[7] += load_real(a.normals, a.normals_f64, b + 1); s[8] += load_real(a.normals, a.normals_f64, b + 2); }
}

__device__ __forceinline__ void voxel_write_row(const VoxelEmit& a, uint32_t v, uint32_t row, const VoxelRange& r, const double (&s)[9]) {
    const double members = (double)(r.end - r.begin);
    const size_t o = 3 * (size_t)row;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out_points[o + k] = (float)(s[k] / members);
        if (a.colors && a.out_colors) a.out_colors[o + k] = (float)(s[3 + k] / members);
        if (a.normals && a.out_normals) a.out_normals[o + k] = (float)(s[6 + k] / members);
    }
    if (a.out_labels) a.out_labels[row] = a.vlabel[v];
    if (a.out_counts) a.out_counts[row] = (int32_t)(r.end - r.begin);
    if (a.out_index) a.out_index[row] = a.sorted_index[r.begin];
}

// one lane per voxel: the kept voxels of at most heavy_from members
__global__ __launch_bounds__(kVoxelThreads) void voxel_emit_kernel(VoxelEmit a) {
    const uint32_t v = blockIdx.x * (uint32_t)kVoxelThreads + threadIdx.x;
    const uint32_t nv = a.meta[0] < a.n ? a.meta[0] : a.n;
    if (v >= nv || a.vlabel[v] < 0) return;
    const uint32_t row = a.row[v];
    if (row >= a.rows) return;
    const VoxelRange r = voxel_range(a.start, v, nv, a.n);
    if (r.end == r.begin || r.end - r.begin > (uint32_t)a.heavy_from) return;
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = r.begin; i < r.end; ++i) {
        const uint32_t j = a.perm[i];
        if (j < a.n) voxel_add_member(a, j, s);
    }
    voxel_write_row(a, v, row, r, s);
}

// a wave per queued voxel: lane l adds members l, l + 64, ..., then a butterfly over the lanes (every lane ends with the same sum)
__global__ __launch_bounds__(kVoxelThreads) void voxel_emit_heavy_kernel(VoxelEmit a, const uint32_t* __restrict__ heavy, uint32_t heavy_capacity) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t nv = a.meta[0] < a.n ? a.meta[0] : a.n;
    const uint32_t n_heavy = a.meta[3] < heavy_capacity ? a.meta[3] : heavy_capacity;
    const uint32_t n_waves = gridDim.x * (uint32_t)(kVoxelThreads / 64);
    for (uint32_t h = blockIdx.x * (uint32_t)(kVoxelThreads / 64) + (uint32_t)w; h < n_heavy; h += n_waves) {   // (wave-uniform)
        const uint32_t v = heavy[h];
        if (v >= nv || a.vlabel[v] < 0) continue;
        const uint32_t row = a.row[v];
        if (row >= a.rows) continue;
        const VoxelRange r = voxel_range(a.start, v, nv, a.n);
        if (r.end == r.begin) continue;
        double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t i = r.begin + (uint32_t)lane; i < r.end; i += 64u) {
            const uint32_t j = a.perm[i];
            if (j < a.n) voxel_add_member(a, j, s);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            for (int m = 32; m > 0; m >>= 1) s[k] += __shfl_xor(s[k], m);
        }
        if (lane == 0) voxel_write_row(a, v, row, r, s);
    }
}

// ---- the launchers ----------------------------------------------------------------------------------------------------------------------
static dim3 voxel_grid(uint32_t n) { return dim3((n + kVoxelThreads - 1) / kVoxelThreads); }
static int voxel_bound_blocks(uint32_t n) { return (int)((n + (uint32_t)kVoxelBoundChunk - 1u) / (uint32_t)kVoxelBoundChunk); }
static uint32_t voxel_heavy_capacity(uint32_t n) { return n / (uint32_t)kVoxelHeavy + 1u; }   // more voxels than that cannot have > kVoxelHeavy members

// index, label8, w0..w2: what the key kernel writes;  ka, kb: a gathered word and a sort's keys_out;  perm, perm_b: the permutation's two
// buffers (the last sort always ends in perm);  sorted_index, sorted_label: after the sort.  Dead once the sorts are done and reused:
// w0 = heads -> voxel ids, w1 = start, w2 = keep -> row, ka = vlabel.
struct VoxelLayout {
    size_t meta, partials, index, label8, w0, w1, w2, ka, kb, perm, perm_b, sorted_index, sorted_label, heavy, chunks, sort_temp, total;
};
static VoxelLayout voxel_layout(uint32_t n) {
    VoxelLayout L;
    Carver c;
    const size_t p = n > 0 ? n : 1;
    L.meta = c.take(16);
    L.partials = c.take(7 * 8 * (size_t)voxel_bound_blocks((uint32_t)p));
    L.index = c.take(8 * p);
    L.label8 = c.take(p);
    L.w0 = c.take(4 * p);
    L.w1 = c.take(4 * p);
    L.w2 = c.take(4 * p);
    L.ka = c.take(4 * p);
    L.kb = c.take(4 * p);
    L.perm = c.take(4 * p);
    L.perm_b = c.take(4 * p);
    L.sorted_index = c.take(8 * p);
    L.sorted_label = c.take(p);
    L.heavy = c.take(4 * (size_t)voxel_heavy_capacity((uint32_t)p));
    L.chunks = c.take(4 * scan_in_place_chunk_words((uint32_t)p));
    L.sort_temp = c.take(radix_sort_temp_bytes((uint32_t)p));
    L.total = c.off;
    return L;
}
static size_t voxel_workspace_bytes(uint32_t n) { return voxel_layout(n).total; }

// n >= 1.  bounds: device [7] doubles
static hipError_t voxel_bounds(uint32_t n, const void* points, int points_f64, void* ws, double* bounds, hipStream_t s) {
    double* partials = at<double>(ws, voxel_layout(n).partials);
    const int nb = voxel_bound_blocks(n);
    hipLaunchKernelGGL(voxel_bounds_kernel, dim3(nb), dim3(kVoxelThreads), 0, s, n, points, points_f64, partials);
    hipLaunchKernelGGL(voxel_bounds_finalize_kernel, dim3(1), dim3(kVoxelThreads), 0, s, partials, nb, bounds);
    return hipGetLastError();
}

static int bits_of(unsigned long long x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }

// n >= 1, 1 <= offset < 2^21.  counts (device, may be nullptr): {voxels, kept, bad labels}
static hipError_t voxel_group(uint32_t n, const void* points, int points_f64, const void* labels, int label_bytes, const double* lo, double voxel_size,
                       long long offset, void* ws, uint32_t* counts, RankMode rank_mode, hipStream_t s) {
    const VoxelLayout L = voxel_layout(n);
    uint32_t* meta = at<uint32_t>(ws, L.meta);
    long long* index = at<long long>(ws, L.index);
    uint8_t* label8 = at<uint8_t>(ws, L.label8);
    uint32_t *w[3] = {at<uint32_t>(ws, L.w0), at<uint32_t>(ws, L.w1), at<uint32_t>(ws, L.w2)};
    uint32_t *ka = at<uint32_t>(ws, L.ka), *kb = at<uint32_t>(ws, L.kb), *perm = at<uint32_t>(ws, L.perm), *perm_b = at<uint32_t>(ws, L.perm_b);
    long long* sorted_index = at<long long>(ws, L.sorted_index);
    uint8_t* sorted_label = at<uint8_t>(ws, L.sorted_label);
    uint32_t* chunks = at<uint32_t>(ws, L.chunks);
    void* sort_temp = at<char>(ws, L.sort_temp);
    const size_t sort_bytes = radix_sort_temp_bytes(n);

    hipError_t e = hipMemsetAsync(meta, 0, 16, s);
    if (e != hipSuccess) return e;
    const VoxelFrame f{{lo[0], lo[1], lo[2]}, voxel_size, offset, labels ? 8 : 0, label_bytes};
    if (points_f64)
        hipLaunchKernelGGL(voxel_key_kernel<double>, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, static_cast<const double*>(points), labels, f, index, label8,
                           w[0], w[1], w[2], meta + 2);
    else
        hipLaunchKernelGGL(voxel_key_kernel<float>, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, static_cast<const float*>(points), labels, f, index, label8,
                           w[0], w[1], w[2], meta + 2);

    // the sort: (label | index) as up to three 32-bit words, the lowest first; a small scene pays few passes
    const unsigned long long o = (unsigned long long)offset;
    int total_bits = f.label_bits + (bits_of(o * o * o - 1ull) > 0 ? bits_of(o * o * o - 1ull) : 1);
    const int n_sorts = (total_bits + 31) / 32;
    uint32_t* out = (n_sorts & 1) ? perm : perm_b;       // ping-pong that ends in perm
    const uint32_t* in = nullptr;                        // the first sort's value is the point's index
    for (int k = 0; k < n_sorts; ++k) {
        const int bits = total_bits > 32 ? 32 : total_bits;
        const uint32_t* keys = w[k];
        if (k > 0) {
            hipLaunchKernelGGL(voxel_gather_words_kernel, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, w[k], in, ka);
            keys = ka;
        }
        e = radix_sort_pairs(keys, in, kb, out, n, bits, sort_temp, sort_bytes, s, nullptr, nullptr, rank_mode, false);
        if (e != hipSuccess) return e;
        in = out;
        out = out == perm ? perm_b : perm;
        total_bits -= bits;
    }
    hipLaunchKernelGGL(voxel_sorted_kernel, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, index, label8, perm, sorted_index, sorted_label);

    uint32_t *voxel_id = w[0], *start = w[1], *keep = w[2];
    int32_t* vlabel = reinterpret_cast<int32_t*>(ka);
    hipLaunchKernelGGL(voxel_heads_kernel, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, sorted_index, voxel_id);
    e = exclusive_scan_in_place(voxel_id, n, chunks, meta, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(voxel_starts_kernel, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, sorted_index, voxel_id, start);
    uint32_t* heavy = at<uint32_t>(ws, L.heavy);
    const uint32_t cap = voxel_heavy_capacity(n);
    hipLaunchKernelGGL(voxel_stats_kernel, voxel_grid(n), dim3(kVoxelThreads), 0, s, n, labels ? 1 : 0, kVoxelHeavy, start, sorted_label, meta, keep, vlabel,
                       heavy, cap);
    if (labels && n > (uint32_t)kVoxelHeavy) {
        const uint32_t blocks = (cap + 3u) / 4u < (uint32_t)kVoxelHeavyBlocks ? (cap + 3u) / 4u : (uint32_t)kVoxelHeavyBlocks;
        hipLaunchKernelGGL(voxel_stats_heavy_kernel, dim3(blocks), dim3(kVoxelThreads), 0, s, n, start, sorted_label, meta, keep, vlabel, heavy, cap);
    }
    e = exclusive_scan_in_place(keep, n, chunks, meta + 1, s);
    if (e != hipSuccess) return e;
    if (counts) e = hipMemcpyAsync(counts, meta, 12, hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// after voxel_group on the same points and workspace; rows >= 1: the kept count the caller read back
static hipError_t voxel_emit(uint32_t n, const void* points, int points_f64, const void* colors, int colors_f64, const void* normals, int normals_f64,
                      const void* ws, uint32_t n_voxels, uint32_t rows, float* out_points, float* out_colors, float* out_normals, int32_t* out_labels,
                      int32_t* out_counts, int64_t* out_index, hipStream_t s) {
    const VoxelLayout L = voxel_layout(n);
    void* base = const_cast<void*>(ws);
    const VoxelEmit a{n, rows, kVoxelHeavy, points, colors, normals, points_f64, colors_f64, normals_f64,
                      at<const uint32_t>(base, L.perm), at<const uint32_t>(base, L.w1), at<const uint32_t>(base, L.w2), at<const uint32_t>(base, L.meta),
                      at<const int32_t>(base, L.ka), at<const long long>(base, L.sorted_index),
                      out_points, out_colors, out_normals, out_labels, out_counts, reinterpret_cast<long long*>(out_index)};
    hipLaunchKernelGGL(voxel_emit_kernel, voxel_grid(n_voxels < n ? n_voxels : n), dim3(kVoxelThreads), 0, s, a);
    if (n > (uint32_t)kVoxelHeavy) {
        const uint32_t cap = voxel_heavy_capacity(n);
        const uint32_t blocks = (cap + 3u) / 4u < (uint32_t)kVoxelHeavyBlocks ? (cap + 3u) / 4u : (uint32_t)kVoxelHeavyBlocks;
        hipLaunchKernelGGL(voxel_emit_heavy_kernel, dim3(blocks), dim3(kVoxelThreads), 0, s, a, at<const uint32_t>(base, L.heavy), cap);
    }
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks the three launching sr_voxel_* calls share: the cloud and the workspace
static int voxel_arguments(int32_t n, const void* points, int32_t points_f64, const void* workspace, size_t workspace_bytes) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n %d is negative", n);
    if (int rc = check_f32_or_f64("points", nullptr, points_f64)) return rc;   // the flag; the address once there are points
    if (n == 0) return SR_OK;
    if (!points) return fail(SR_ERR_INVALID_ARGUMENT, "points is NULL");
    if (int rc = check_f32_or_f64("points", points, points_f64)) return rc;
    return check_workspace(workspace, workspace_bytes, voxel_workspace_bytes((uint32_t)n));
}

extern "C" {

size_t sr_voxel_workspace_bytes(int32_t n) { return n < 0 ? 0 : voxel_workspace_bytes((uint32_t)n); }

int sr_voxel_bounds(int32_t n, const void* points, int32_t points_f64, void* workspace, size_t workspace_bytes, double* bounds, void* stream) {
    if (int rc = voxel_arguments(n, points, points_f64, workspace, workspace_bytes)) return rc;
    if (!bounds) return fail(SR_ERR_INVALID_ARGUMENT, "bounds is NULL");
    if ((uintptr_t)bounds & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "bounds is not 8-B aligned");
    if (n == 0) return fail(SR_ERR_INVALID_ARGUMENT, "an empty cloud has no bounds");
    SR_HIP(voxel_bounds((uint32_t)n, points, points_f64, workspace, bounds, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_voxel_group(int32_t n, const void* points, int32_t points_f64, const void* semantics, int32_t semantics_bytes, const double* lo,
                   double voxel_size, int64_t offset, void* workspace, size_t workspace_bytes, uint32_t* counts, void* stream) {
    if (int rc = voxel_arguments(n, points, points_f64, workspace, workspace_bytes)) return rc;
    if (!(voxel_size > 0.0 && voxel_size <= DBL_MAX)) return fail(SR_ERR_INVALID_ARGUMENT, "voxel_size %g is not a positive finite number", voxel_size);
    if (!lo) return fail(SR_ERR_INVALID_ARGUMENT, "lo is NULL");
    if (!(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2])))
        return fail(SR_ERR_INVALID_ARGUMENT, "lo = (%g, %g, %g) is not finite: the cloud has a NaN or infinite coordinate", lo[0], lo[1], lo[2]);
    if (offset < 1) return fail(SR_ERR_INVALID_ARGUMENT, "offset %lld < 1", (long long)offset);
    if (offset >= kVoxelMaxOffset)
        return fail(SR_ERR_UNSUPPORTED, "offset %lld >= 2^21: offset^3 would leave int64 (a larger voxel_size, or the cloud in parts)", (long long)offset);
    if (semantics && semantics_bytes != 4 && semantics_bytes != 8) return fail(SR_ERR_INVALID_ARGUMENT, "semantics_bytes = %d: 4 (int32) or 8 (int64)", semantics_bytes);
    if (semantics && ((uintptr_t)semantics & (uintptr_t)(semantics_bytes - 1))) return fail(SR_ERR_INVALID_ARGUMENT, "semantics is not aligned to its element size");
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if ((uintptr_t)counts & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "counts is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) { SR_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), s)); return SR_OK; }
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(s, false, &sort_mode)) return rc;
    SR_HIP(voxel_group((uint32_t)n, points, points_f64, semantics, semantics_bytes, lo, voxel_size, (long long)offset, workspace, counts, sort_mode, s));
    return SR_OK;
}

int sr_voxel_emit(int32_t n, const void* points, int32_t points_f64, const void* colors, int32_t colors_f64, const void* normals,
                  int32_t normals_f64, void* workspace, size_t workspace_bytes, int32_t n_voxels, int32_t n_kept, float* out_points,
                  float* out_colors, float* out_normals, int32_t* out_semantics, int32_t* out_counts, int64_t* out_index, void* stream) {
    if (int rc = voxel_arguments(n, points, points_f64, workspace, workspace_bytes)) return rc;
    if (int rc = check_f32_or_f64("colors", colors, colors_f64)) return rc;
    if (int rc = check_f32_or_f64("normals", normals, normals_f64)) return rc;
    if (n_voxels < 0 || n_voxels > n) return fail(SR_ERR_INVALID_ARGUMENT, "n_voxels = %d: not in 0..n = %d", n_voxels, n);
    if (n_kept < 0 || n_kept > n_voxels) return fail(SR_ERR_INVALID_ARGUMENT, "n_kept = %d: not in 0..n_voxels = %d", n_kept, n_voxels);
    if (n_kept == 0) return SR_OK;
    if (!out_points) return fail(SR_ERR_INVALID_ARGUMENT, "out_points is NULL");
    if (colors && !out_colors) return fail(SR_ERR_INVALID_ARGUMENT, "out_colors is NULL (colors is given)");
    if (normals && !out_normals) return fail(SR_ERR_INVALID_ARGUMENT, "out_normals is NULL (normals is given)");
    if (((uintptr_t)out_points | (uintptr_t)out_colors | (uintptr_t)out_normals | (uintptr_t)out_semantics | (uintptr_t)out_counts) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "an output is not 4-B aligned");
    if ((uintptr_t)out_index & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "out_index is not 8-B aligned");
    SR_HIP(voxel_emit((uint32_t)n, points, points_f64, colors, colors_f64, normals, normals_f64, workspace, (uint32_t)n_voxels, (uint32_t)n_kept, out_points,
                      out_colors, out_normals, out_semantics, out_counts, out_index, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
