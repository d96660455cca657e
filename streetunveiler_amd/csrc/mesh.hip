// mesh.hip -- marching cubes on a resident float32 volume [nx,ny,nz] (iz fastest: what sr_tsdf_fuse_grid fills) -> an indexed, welded
// triangle mesh (include/surfel_raster.h states the semantics; mc_table.h the case table and its conventions):
//   mesh_count_kernel      one thread per grid point, kMeshRows points a thread: the vertices the point owns (its three forward edges)
//                          and the triangles of the cell whose lowest corner it is; one (vertices, triangles) sum per chunk of 4096 points
//   mesh_totals_kernel     exclusive scan of the chunk sums (one block); the two totals, taken in 64 bits, go to the caller's device words
//   mesh_vertices_kernel   the flags again, scanned inside the chunk: every owned vertex at its offset; the offset and the flags of every
//                          owning point stay in the workspace (4 + 1 bytes a grid point)
//   mesh_faces_kernel      the cases again, scanned inside the chunk: every triangle's three edges -> (owning point, axis) -> the owner's
//                          offset + the rank of the axis among the owner's flags
// A vertex is identified by (owning grid point, axis): welding is the prefix sum, there is no hashing and there are no atomics -- equal
// inputs give equal bits; vertices ascend by (linear point index, axis), faces by (linear cell index, table order).  A chunk without
// vertices (triangles) leaves its emission kernel at once: on a fused TSDF, which is +-1 away from the surface, that is most of them.
// Built with -ffp-contract=off: the only fused operations are the fmaf()s of the coordinates; t is the correctly rounded quotient.
#include <cmath>

#include "contraction.h"
#include "abi.h"
#include "mc_table.h"
#include "scan.h"

namespace sr {

constexpr int kMeshThreads = 256;
constexpr int kMeshRows = 16;                              // rows of kMeshThreads consecutive points a block walks
constexpr int kMeshChunk = kMeshThreads * kMeshRows;       // 4096 points: at most 12288 vertices and 20480 triangles, 16 bits each
constexpr int kMeshScanThreads = 1024;

struct MeshGrid {          // kernel parameters, by value
    int nx, ny, nz;        // every axis at least 2 (a grid without cells never reaches a launch)
    uint32_t n;            // nx ny nz < 2^31
    float level;
};
struct MeshFrame {         // grid point (ix, iy, iz) sits at fmaf(index, step, lo) per axis
    float lo[3], step[3];
};

struct MeshLayout {
    size_t offsets, flags, chunks, total;
    uint32_t nchunks;
};
static MeshLayout mesh_layout(uint32_t n) {
    MeshLayout L;
    L.nchunks = (uint32_t)(((size_t)n + kMeshChunk - 1) / kMeshChunk);
    Carver c;
    L.offsets = c.take(4 * (size_t)n);
    L.flags = c.take((size_t)n);
    L.chunks = c.take(16 * ((size_t)L.nchunks + 1));
    L.total = c.off;
    return L;
}
static size_t mesh_workspace_bytes(uint32_t n) { return mesh_layout(n).total; }

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }   // (a NaN compares false)

struct MeshPoint {
    uint32_t i;
    int ix, iy, iz;
};
__device__ __forceinline__ MeshPoint mesh_point(const MeshGrid& g, uint32_t i) {
    const uint32_t plane = (uint32_t)g.ny * (uint32_t)g.nz;
    const uint32_t ix = i / plane, rem = i - ix * plane, iy = rem / (uint32_t)g.nz;
    return MeshPoint{i, (int)ix, (int)iy, (int)(rem - iy * (uint32_t)g.nz)};
}

// Bit a: the edge from the point along axis a holds a vertex -- both ends finite, exactly one of them inside (value < level).
// v0 and the three forward neighbours are handed back for the interpolation (a neighbour outside the grid reads as NaN: no edge).
__device__ __forceinline__ uint32_t owned_vertices(const float* __restrict__ vol, const MeshGrid& g, const MeshPoint& p, float& v0, float& vx, float& vy,
                                                   float& vz) {
    const size_t at = p.i, plane = (size_t)g.ny * (size_t)g.nz;
    v0 = vol[at];
    vx = p.ix + 1 < g.nx ? vol[at + plane] : NAN;
    vy = p.iy + 1 < g.ny ? vol[at + (size_t)g.nz] : NAN;
    vz = p.iz + 1 < g.nz ? vol[at + 1] : NAN;
    if (!is_finite(v0)) return 0u;
    const bool in0 = v0 < g.level;
    return (is_finite(vx) && in0 != (vx < g.level) ? 1u : 0u) | (is_finite(vy) && in0 != (vy < g.level) ? 2u : 0u) |
           (is_finite(vz) && in0 != (vz < g.level) ? 4u : 0u);
}

// The case of the cell whose lowest corner the point is: bit c = corner c inside; 0 (no triangle) where there is no such cell or one
// of its corners is not finite.
__device__ __forceinline__ uint32_t cell_case(const float* __restrict__ vol, const MeshGrid& g, const MeshPoint& p) {
    if (!(p.ix + 1 < g.nx && p.iy + 1 < g.ny && p.iz + 1 < g.nz)) return 0u;
    const size_t plane = (size_t)g.ny * (size_t)g.nz;
    uint32_t bits = 0u;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float v = vol[(size_t)p.i + (size_t)(c & 1) * plane + (size_t)((c >> 1) & 1) * (size_t)g.nz + (size_t)(c >> 2)];
        finite = finite && is_finite(v);
        bits |= (v < g.level ? 1u : 0u) << c;
    }
    return finite ? bits : 0u;
}

__global__ __launch_bounds__(kMeshThreads) void mesh_count_kernel(const float* __restrict__ vol, const MeshGrid g, uint4* __restrict__ chunk_total) {
    __shared__ uint8_t s_count[256];
    __shared__ uint32_t s_w[kMeshThreads / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kMeshChunk;   // n < 2^31: base + 4095 does not overflow
    s_count[tid] = kMcTriCount[tid];
    __syncthreads();
    uint32_t packed = 0u;   // vertices | triangles << 16
    for (int r = 0; r < kMeshRows; ++r) {
        const uint32_t i = base + (uint32_t)r * kMeshThreads + tid;
        if (i >= g.n) break;
        const MeshPoint p = mesh_point(g, i);
        float v0, vx, vy, vz;
        packed += (uint32_t)__popc(owned_vertices(vol, g, p, v0, vx, vy, vz)) + ((uint32_t)s_count[cell_case(vol, g, p)] << 16);
    }
    uint32_t total;
    block_exclusive_scan<kMeshThreads / 64>(packed, s_w, total);   // (only the total is used)
    if (tid == 0) chunk_total[blockIdx.x] = make_uint4(total & 0xFFFFu, total >> 16, 0u, 0u);
}

// exclusive scan of chunk_total[0 .. nchunks) in place, one block; chunk_total[nchunks] = the totals, so that chunk k's own sums are
// the difference of entries k + 1 and k.  counts = {Nv, Nf}, 0xFFFFFFFF where Nv or 3 Nf is beyond int32 (the 32-bit scan is void then).
__global__ __launch_bounds__(kMeshScanThreads) void mesh_totals_kernel(uint4* __restrict__ chunk_total, int nchunks, uint32_t* __restrict__ counts) {
    __shared__ uint4 s_w[kMeshScanThreads / 64];
    __shared__ unsigned long long s_v[kMeshScanThreads], s_t[kMeshScanThreads];
    const int tid = threadIdx.x;
    unsigned long long v = 0ull, t = 0ull;
    for (int k = tid; k < nchunks; k += kMeshScanThreads) { const uint4 c = chunk_total[k]; v += c.x; t += c.y; }
    s_v[tid] = v; s_t[tid] = t;
    __syncthreads();
    for (int half = kMeshScanThreads / 2; half > 0; half >>= 1) {
        if (tid < half) { s_v[tid] += s_v[tid + half]; s_t[tid] += s_t[tid + half]; }
        __syncthreads();
    }
    const uint4 total = carried_exclusive_scan<kMeshScanThreads / 64>(chunk_total, nchunks, s_w);
    if (tid == 0) {
        chunk_total[nchunks] = total;
        counts[0] = s_v[0] > 0x7FFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s_v[0];
        counts[1] = 3ull * s_t[0] > 0x7FFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s_t[0];
    }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_vertices_kernel(const float* __restrict__ vol, const MeshGrid g, const MeshFrame fr, const TsdfSpace space,
                                                                     const uint4* __restrict__ chunk_base, uint32_t* __restrict__ offsets,
                                                                     uint8_t* __restrict__ flags, uint32_t n_vertices, float* __restrict__ vertices) {
    __shared__ uint32_t s_w[kMeshThreads / 64];
    uint32_t carry = chunk_base[blockIdx.x].x;
    if (chunk_base[blockIdx.x + 1].x == carry) return;   // the whole block: a chunk that owns no vertex
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kMeshChunk;
    for (int r = 0; r < kMeshRows; ++r) {
        if (base + (uint32_t)r * kMeshThreads >= g.n) break;   // the whole block
        const uint32_t i = base + (uint32_t)r * kMeshThreads + tid;
        MeshPoint p{};
        float v0 = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
        uint32_t f = 0u;
        if (i < g.n) { p = mesh_point(g, i); f = owned_vertices(vol, g, p, v0, vx, vy, vz); }
        uint32_t total;
        uint32_t at = carry + block_exclusive_scan<kMeshThreads / 64>((uint32_t)__popc(f), s_w, total);
        carry += total;
        if (!f) continue;
        offsets[i] = at;
        flags[i] = (uint8_t)f;
        const float gx = fmaf((float)p.ix, fr.step[0], fr.lo[0]), gy = fmaf((float)p.iy, fr.step[1], fr.lo[1]), gz = fmaf((float)p.iz, fr.step[2], fr.lo[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(f & (1u << a))) continue;
            const float vb = a == 0 ? vx : a == 1 ? vy : vz;
            const float t = __fdiv_rn(g.level - v0, vb - v0);   // v0: the value at the lower-index end
            float x = gx, y = gy, z = gz;
            if (a == 0) x = fmaf((float)p.ix + t, fr.step[0], fr.lo[0]);
            else if (a == 1) y = fmaf((float)p.iy + t, fr.step[1], fr.lo[1]);
            else z = fmaf((float)p.iz + t, fr.step[2], fr.lo[2]);
            if (space.contract) uncontract_to_world(x, y, z, space);
            if (at < n_vertices) { vertices[3 * (size_t)at] = x; vertices[3 * (size_t)at + 1] = y; vertices[3 * (size_t)at + 2] = z; }
            ++at;
        }
    }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_faces_kernel(const float* __restrict__ vol, const MeshGrid g, const uint4* __restrict__ chunk_base,
                                                                  const uint32_t* __restrict__ offsets, const uint8_t* __restrict__ flags,
                                                                  uint32_t n_faces, int32_t* __restrict__ faces) {
    __shared__ uint8_t s_count[256], s_edges[256 * 3 * kMcMaxTriangles], s_owner[12];
    __shared__ uint32_t s_w[kMeshThreads / 64];
    uint32_t carry = chunk_base[blockIdx.x].y;
    if (chunk_base[blockIdx.x + 1].y == carry) return;   // the whole block: a chunk without a triangle
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kMeshChunk;
    s_count[tid] = kMcTriCount[tid];
    for (int k = (int)tid; k < 256 * 3 * kMcMaxTriangles; k += kMeshThreads) s_edges[k] = kMcTriEdges[k];
    if (tid < 12) s_owner[tid] = kMcEdgeOwner[tid];
    __syncthreads();
    const size_t plane = (size_t)g.ny * (size_t)g.nz;
    for (int r = 0; r < kMeshRows; ++r) {
        if (base + (uint32_t)r * kMeshThreads >= g.n) break;   // the whole block
        const uint32_t i = base + (uint32_t)r * kMeshThreads + tid;
        const uint32_t mc = i < g.n ? cell_case(vol, g, mesh_point(g, i)) : 0u;
        const uint32_t nt = s_count[mc];
        uint32_t total;
        const uint32_t first = carry + block_exclusive_scan<kMeshThreads / 64>(nt, s_w, total);
        carry += total;
        for (uint32_t k = 0; k < nt; ++k) {
            if (first + k >= n_faces) break;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t owner = s_owner[s_edges[mc * (3 * kMcMaxTriangles) + 3 * k + j]];   // a crossed edge of a cell with finite corners
                const size_t at = (size_t)i + (size_t)(owner & 1u) * plane + (size_t)((owner >> 1) & 1u) * (size_t)g.nz + (size_t)((owner >> 2) & 1u);
                const uint32_t below = (1u << (owner >> 3)) - 1u;   // the owner's flags of the axes before this one
                faces[3 * (size_t)(first + k) + j] = (int32_t)(offsets[at] + (uint32_t)__popc((uint32_t)flags[at] & below));
            }
        }
    }
}

// counts: device {Nv, Nf}; a count is 0xFFFFFFFF where Nv or 3 Nf is beyond int32
static hipError_t mesh_count(const float* volume, const MeshGrid& g, void* workspace, uint32_t* counts, hipStream_t s) {
    const MeshLayout L = mesh_layout(g.n);
    uint4* chunks = at<uint4>(workspace, L.chunks);
    hipLaunchKernelGGL(mesh_count_kernel, dim3(L.nchunks), dim3(kMeshThreads), 0, s, volume, g, chunks);
    hipLaunchKernelGGL(mesh_totals_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, chunks, (int)L.nchunks, counts);
    return hipGetLastError();
}

// after mesh_count on the same volume, level and workspace; space.contract: the vertices are un-contracted and un-normalised
static hipError_t mesh_emit(const float* volume, const MeshGrid& g, const MeshFrame& frame, const TsdfSpace& space, void* workspace, uint32_t n_vertices,
                     uint32_t n_faces, float* vertices, int32_t* faces, hipStream_t s) {
    const MeshLayout L = mesh_layout(g.n);
    const uint4* chunks = at<uint4>(workspace, L.chunks);
    uint32_t* offsets = at<uint32_t>(workspace, L.offsets);
    uint8_t* flags = at<uint8_t>(workspace, L.flags);
    if (n_vertices > 0)
        hipLaunchKernelGGL(mesh_vertices_kernel, dim3(L.nchunks), dim3(kMeshThreads), 0, s, volume, g, frame, space, chunks, offsets, flags, n_vertices, vertices);
    if (n_faces > 0)
        hipLaunchKernelGGL(mesh_faces_kernel, dim3(L.nchunks), dim3(kMeshThreads), 0, s, volume, g, chunks, offsets, flags, n_faces, faces);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks sr_mesh_count and sr_mesh_emit share -> the kernels' view of the grid; *cells = 0 for a grid with an axis of length 1
static int mesh_arguments(const float* volume, const int32_t* dims, float level, const void* workspace, size_t workspace_bytes, MeshGrid* g, bool* cells) {
    if (!volume) return fail(SR_ERR_INVALID_ARGUMENT, "volume is NULL");
    if (!dims) return fail(SR_ERR_INVALID_ARGUMENT, "dims is NULL");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(SR_ERR_INVALID_ARGUMENT, "dims %d x %d x %d: every axis holds at least one sample", dims[0], dims[1], dims[2]);
    if (level != level) return fail(SR_ERR_INVALID_ARGUMENT, "level is NaN");
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];   // < 2^62: the product below cannot wrap
    const unsigned long long n = plane < (1ull << 31) ? plane * (unsigned long long)dims[2] : plane;
    if (n >= (1ull << 31))
        return fail(SR_ERR_UNSUPPORTED, "a grid of %d x %d x %d points: fewer than 2^31", dims[0], dims[1], dims[2]);
    // (a short workspace is an invalid argument here, not SR_ERR_BUFFER_TOO_SMALL as everywhere else: what these two calls have always returned)
    if (int rc = check_workspace(workspace, workspace_bytes, mesh_workspace_bytes((uint32_t)n), SR_ERR_INVALID_ARGUMENT)) return rc;
    if ((uintptr_t)volume & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "volume is not 4-B aligned");
    *g = MeshGrid{dims[0], dims[1], dims[2], (uint32_t)n, level};
    *cells = dims[0] > 1 && dims[1] > 1 && dims[2] > 1;
    return SR_OK;
}

extern "C" {

size_t sr_mesh_workspace_bytes(const int32_t* dims) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return 0;
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane >= (1ull << 31) || plane * (unsigned long long)dims[2] >= (1ull << 31)) return 0;
    return mesh_workspace_bytes((uint32_t)(plane * (unsigned long long)dims[2]));
}

int sr_mesh_count(const float* volume, const int32_t* dims, float level, void* workspace, size_t workspace_bytes, uint32_t* counts, void* stream) {
    MeshGrid g; bool cells;
    if (int rc = mesh_arguments(volume, dims, level, workspace, workspace_bytes, &g, &cells)) return rc;
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if ((uintptr_t)counts & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "counts is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!cells) { SR_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s)); return SR_OK; }
    SR_HIP(mesh_count(volume, g, workspace, counts, s));
    return SR_OK;
}

int sr_mesh_emit(const float* volume, const int32_t* dims, float level, const float* lo, const float* step, const SrTsdfSpace* space,
                 void* workspace, size_t workspace_bytes, int32_t n_vertices, int32_t n_faces, float* vertices, int32_t* faces, void* stream) {
    MeshGrid g; bool cells;
    if (int rc = mesh_arguments(volume, dims, level, workspace, workspace_bytes, &g, &cells)) return rc;
    if (!lo || !step) return fail(SR_ERR_INVALID_ARGUMENT, "lo / step is NULL");
    if (n_vertices < 0 || n_faces < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n_vertices %d / n_faces %d is negative", n_vertices, n_faces);
    if (n_faces > 0x7FFFFFFF / 3) return fail(SR_ERR_UNSUPPORTED, "%d faces: 3 n_faces does not fit in int32", n_faces);
    if (n_faces > 0 && n_vertices == 0) return fail(SR_ERR_INVALID_ARGUMENT, "%d faces without vertices", n_faces);
    if (n_vertices > 0 && !vertices) return fail(SR_ERR_INVALID_ARGUMENT, "vertices is NULL");
    if (n_faces > 0 && !faces) return fail(SR_ERR_INVALID_ARGUMENT, "faces is NULL");
    if (((uintptr_t)vertices | (uintptr_t)faces) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "vertices / faces is not 4-B aligned");
    if (!cells || n_vertices == 0) return SR_OK;
    const MeshFrame frame{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}};
    TsdfSpace sp{0.f, 0, {0.f, 0.f, 0.f}, 1.f};
    if (space && space->contract) sp = TsdfSpace{0.f, 1, {space->center[0], space->center[1], space->center[2]}, space->radius};
    SR_HIP(mesh_emit(volume, g, frame, sp, workspace, (uint32_t)n_vertices, (uint32_t)n_faces, vertices, faces, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
