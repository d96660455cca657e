// mesh_post.hip -- the post-processing of an indexed triangle mesh (faces [nf,3] int32 over nv vertices; include/surfel_raster.h states the
// semantics): the edge-connected components of the faces, then the mesh without the faces of the small components, without the vertices
// no remaining face references and without the faces that name a vertex twice.
//
// Edge matching, without a sort: a half-edge (face f, corner j) runs between the vertices lo <= hi.  The 3 nf half-edges are bucketed by
// lo -- a degree count with integer atomics, one exclusive scan (scan.h), a fill through the scanned offsets themselves, which the fill
// advances from the begin of every bucket to its end -- and every half-edge then walks the bucket of its lo and unites its face with the
// face of the FIRST entry that has its hi (union_find.h).  All the faces on one edge are thereby joined to one of them, whichever winding
// they have and however many they are.  The order of the entries inside a bucket depends on how the fill's atomics raced; the labels do
// not: whichever entry comes first, the unions join exactly the faces with an equal edge, and the root of a finished tree is the
// smallest face index of its component.  The sizes are integer sums, the compaction is two exclusive scans: equal inputs, equal bits.
//
// Cost: a half-edge reads at most the entries of its bucket, so a vertex of valence d costs up to (2 d)^2 / 2 entry reads.  On a
// marching-cubes mesh d is about 6 and a bucket holds about 6 entries of 8 bytes, one or two cache lines; a hub vertex (a closed fan of
// 3000 faces: 18 million reads by 6000 lanes) is slow and still right.  Two stable passes of the 32-bit radix sort over (hi, lo) would cost
// the same for every mesh; they move 3 nf pairs four times through memory, where this scheme writes them once and reads them from cache,
// so the bucket scheme is the one built (tools/time_mesh_post.py measures it; DESIGN.md quotes the figures).
//
// A face with an index outside [0, nv) is never used to address anything: it takes part in no bucket, stays a component of its own, is
// never kept, and is counted.  Integer / latency work only; no LDS beyond the scans', no MFMA.
#include "abi.h"
#include "scan.h"
#include "union_find.h"

namespace sr {

constexpr int kPostThreads = 256;
constexpr int kPostRows = 16;                              // rows of kPostThreads consecutive items a block of a scan walks
constexpr int kPostChunk = kPostThreads * kPostRows;       // 4096 items a chunk
constexpr int kPostScanThreads = 1024;

// vert: one word a vertex -- the buckets' offsets (components), the used flags and then the new indices (filter)
// edge: one (hi, face) pair a half-edge (components); its head is one word a face, the flags and then the new indices (filter)
// parent: the union-find's forest;  chunks: the sums of a scan's chunks
struct MeshPostLayout {
    size_t vert, edge, parent, chunks, total;
};
static MeshPostLayout mesh_post_layout(int nv, int nf) {
    MeshPostLayout L;
    Carver c;
    const size_t v = nv > 0 ? nv : 1, f = nf > 0 ? nf : 1;
    L.vert = c.take(4 * v);
    L.edge = c.take(8 * 3 * f);
    L.parent = c.take(4 * f);
    L.chunks = c.take(4 * scan_in_place_chunk_words((uint32_t)(v > f ? v : f)));
    L.total = c.off;
    return L;
}
static size_t mesh_post_workspace_bytes(int nv, int nf) { return mesh_post_layout(nv, nf).total; }

// ---- an exclusive scan of n < 2^31 words in place: the sums of the chunks, their scan by one block, the chunks again with their bases ----
__global__ __launch_bounds__(kPostThreads) void post_chunk_sums_kernel(const uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ chunk_sum) {
    __shared__ uint32_t s_w[kPostThreads / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kPostChunk;   // n < 2^31: base + 4095 does not overflow
    uint32_t sum = 0u;
    for (int r = 0; r < kPostRows; ++r) {
        const uint32_t i = base + (uint32_t)r * kPostThreads + tid;
        if (i < n) sum += data[i];
    }
    uint32_t total;
    block_exclusive_scan<kPostThreads / 64>(sum, s_w, total);   // (only the total is used)
    if (tid == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPostScanThreads) void post_chunk_bases_kernel(uint32_t* __restrict__ chunk_sum, int nchunks, uint32_t* __restrict__ total_out) {
    __shared__ uint32_t s_w[kPostScanThreads / 64];
    const uint32_t total = carried_exclusive_scan<kPostScanThreads / 64>(chunk_sum, nchunks, s_w);
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

__global__ __launch_bounds__(kPostThreads) void post_chunk_apply_kernel(uint32_t* __restrict__ data, uint32_t n, const uint32_t* __restrict__ chunk_base) {
    __shared__ uint32_t s_w[kPostThreads / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kPostChunk;
    uint32_t carry = chunk_base[blockIdx.x];
    for (int r = 0; r < kPostRows; ++r) {
        if (base + (uint32_t)r * kPostThreads >= n) break;   // the whole block
        const uint32_t i = base + (uint32_t)r * kPostThreads + tid;
        const uint32_t x = i < n ? data[i] : 0u;
        uint32_t total;
        const uint32_t at = carry + block_exclusive_scan<kPostThreads / 64>(x, s_w, total);
        carry += total;
        if (i < n) data[i] = at;
    }
}

// n >= 1; the sum must fit in 32 bits (here: at most 3 nf, nv or nf); total_out (device, may be nullptr) gets it.  Declared in launch.h:
// unveil.hip compacts with it too.
static_assert(kPostChunk == kScanInPlaceChunk, "launch.h sizes the callers' chunk scratch");
hipError_t exclusive_scan_in_place(uint32_t* data, uint32_t n, uint32_t* chunks, uint32_t* total_out, hipStream_t s) {
    const uint32_t nchunks = (n + kPostChunk - 1) / kPostChunk;
    hipLaunchKernelGGL(post_chunk_sums_kernel, dim3(nchunks), dim3(kPostThreads), 0, s, data, n, chunks);
    hipLaunchKernelGGL(post_chunk_bases_kernel, dim3(1), dim3(kPostScanThreads), 0, s, chunks, (int)nchunks, total_out);
    hipLaunchKernelGGL(post_chunk_apply_kernel, dim3(nchunks), dim3(kPostThreads), 0, s, data, n, chunks);
    return hipGetLastError();
}

// ---- the faces ------------------------------------------------------------------------------------------------------------------------
struct PostFace {
    int a, b, c;
    bool in_range;   // every index in [0, nv): only then is one of them used as an address
};
__device__ __forceinline__ PostFace load_face(const int32_t* __restrict__ faces, int f, int nv) {
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    return PostFace{a, b, c, (uint32_t)a < (uint32_t)nv && (uint32_t)b < (uint32_t)nv && (uint32_t)c < (uint32_t)nv};
}

// every face a tree of its own; the number of half-edges whose lower vertex a vertex is; the faces out of range
__global__ __launch_bounds__(kPostThreads) void post_degree_kernel(const int32_t* __restrict__ faces, int nv, int nf, uint32_t* __restrict__ degree,
                                                                   int* __restrict__ parent, uint32_t* __restrict__ n_bad) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (i >= nf) return;
    const int f = (int)i;
    parent[f] = f;
    const PostFace t = load_face(faces, f, nv);
    if (!t.in_range) { atomicAdd(n_bad, 1u); return; }
    atomicAdd(degree + min(t.a, t.b), 1u);
    atomicAdd(degree + min(t.b, t.c), 1u);
    atomicAdd(degree + min(t.c, t.a), 1u);
}

// cursor[v]: the begin of v's bucket before this kernel, its end after it -- which is the begin of v + 1's
__global__ __launch_bounds__(kPostThreads) void post_fill_kernel(const int32_t* __restrict__ faces, int nv, int nf, uint32_t* __restrict__ cursor,
                                                                 uint2* __restrict__ entries) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (i >= nf) return;
    const int f = (int)i;
    const PostFace t = load_face(faces, f, nv);
    if (!t.in_range) return;
    const uint32_t n_entries = 3u * (uint32_t)nf;
    uint32_t at = atomicAdd(cursor + min(t.a, t.b), 1u);
    if (at < n_entries) entries[at] = make_uint2((uint32_t)max(t.a, t.b), (uint32_t)f);
    at = atomicAdd(cursor + min(t.b, t.c), 1u);
    if (at < n_entries) entries[at] = make_uint2((uint32_t)max(t.b, t.c), (uint32_t)f);
    at = atomicAdd(cursor + min(t.c, t.a), 1u);
    if (at < n_entries) entries[at] = make_uint2((uint32_t)max(t.c, t.a), (uint32_t)f);
}

// One thread per half-edge: the first entry of its bucket with its upper vertex (its own at the latest) names the face it joins.
__global__ __launch_bounds__(kPostThreads) void post_unite_kernel(const int32_t* __restrict__ faces, int nv, int nf, const uint32_t* __restrict__ bucket_end,
                                                                  const uint2* __restrict__ entries, int* parent) {
    const long long e = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (e >= 3ll * nf) return;
    const int f = (int)(e / 3), j = (int)(e - 3ll * f);
    const PostFace t = load_face(faces, f, nv);
    if (!t.in_range) return;
    const int u = j == 0 ? t.a : j == 1 ? t.b : t.c, w = j == 0 ? t.b : j == 1 ? t.c : t.a;
    const int lo = min(u, w);
    const uint32_t hi = (uint32_t)max(u, w), n_entries = 3u * (uint32_t)nf;
    const uint32_t begin = lo > 0 ? bucket_end[lo - 1] : 0u, end = min(bucket_end[lo], n_entries);
    for (uint32_t k = begin; k < end; ++k) {
        const uint2 entry = entries[k];
        if (entry.x != hi) continue;
        const int g = (int)entry.y;
        // on a closed surface most edges join what is joined already: two loads, no atomic
        if (g != f && (uint32_t)g < (uint32_t)nf && load_parent(parent, f) != load_parent(parent, g)) unite(parent, f, g);
        break;
    }
}

// After the unions (the kernel boundary is the fence): the label of every face, and the size of every component at its root.  The lanes
// of a wave that found the same root add their number once.
__global__ __launch_bounds__(kPostThreads) void post_labels_kernel(int nf, int* parent, int32_t* __restrict__ labels, int32_t* __restrict__ sizes) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    const bool valid = i < nf;
    const int lane = threadIdx.x & 63;
    int root = -1;
    if (valid) { root = find_root(parent, (int)i); labels[i] = root; }
    unsigned long long todo = ballot64(valid);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int r = __shfl(root, leader);
        const unsigned long long same = ballot64(valid && root == r);
        if (lane == leader) atomicAdd(sizes + r, (int)__popcll(same));
        todo &= ~same;
    }
}

// keep-face, used-vertex and not-degenerate, in the order the removals run: the faces of the components below *threshold go first, a vertex
// is used by the faces that remain then, the degenerate ones among them included, and those go last.  The used flags are plain stores
// of 1: every writer stores the same value.
__global__ __launch_bounds__(kPostThreads) void post_flags_kernel(const int32_t* __restrict__ faces, int nv, int nf, const int32_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ sizes, const int32_t* __restrict__ threshold,
                                                                  uint32_t* __restrict__ vertex_used, uint32_t* __restrict__ face_kept, uint32_t* __restrict__ n_bad) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (i >= nf) return;
    const int f = (int)i;
    const PostFace t = load_face(faces, f, nv);
    uint32_t kept = 0u;
    if (!t.in_range) {
        atomicAdd(n_bad, 1u);
    } else {
        const int root = labels[f];
        if ((uint32_t)root < (uint32_t)nf && sizes[root] >= *threshold) {
            vertex_used[t.a] = 1u; vertex_used[t.b] = 1u; vertex_used[t.c] = 1u;
            kept = (t.a != t.b && t.b != t.c && t.c != t.a) ? 1u : 0u;
        }
    }
    face_kept[f] = kept;
}

// map[i]: the exclusive scan of the flags; item i has its flag set iff the next entry (the total behind the last) is larger
__device__ __forceinline__ bool post_flagged(const uint32_t* __restrict__ map, uint32_t i, uint32_t n, uint32_t total, uint32_t& at) {
    at = map[i];
    return (i + 1u < n ? map[i + 1u] : total) != at && at < total;
}

// rows are copied word by word: no arithmetic touches them
__global__ __launch_bounds__(kPostThreads) void post_vertices_kernel(const uint32_t* __restrict__ vertex_map, int nv, uint32_t nv_out,
                                                                     const uint32_t* __restrict__ vertices, const uint32_t* __restrict__ colors,
                                                                     uint32_t* __restrict__ vertices_out, uint32_t* __restrict__ colors_out) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (i >= nv) return;
    uint32_t at;
    if (!post_flagged(vertex_map, (uint32_t)i, (uint32_t)nv, nv_out, at)) return;
    const size_t from = 3 * (size_t)i, to = 3 * (size_t)at;
    vertices_out[to] = vertices[from]; vertices_out[to + 1] = vertices[from + 1]; vertices_out[to + 2] = vertices[from + 2];
    if (colors) { colors_out[to] = colors[from]; colors_out[to + 1] = colors[from + 1]; colors_out[to + 2] = colors[from + 2]; }
}

__global__ __launch_bounds__(kPostThreads) void post_faces_kernel(const int32_t* __restrict__ faces, int nv, int nf, const uint32_t* __restrict__ face_map,
                                                                  const uint32_t* __restrict__ vertex_map, uint32_t nf_out, int32_t* __restrict__ faces_out) {
    const long long i = (long long)blockIdx.x * kPostThreads + threadIdx.x;
    if (i >= nf) return;
    uint32_t at;
    if (!post_flagged(face_map, (uint32_t)i, (uint32_t)nf, nf_out, at)) return;
    const PostFace t = load_face(faces, (int)i, nv);   // a kept face is in range (the flags kernel): the test only guards the loads below
    if (!t.in_range) return;
    faces_out[3 * (size_t)at] = (int32_t)vertex_map[t.a];
    faces_out[3 * (size_t)at + 1] = (int32_t)vertex_map[t.b];
    faces_out[3 * (size_t)at + 2] = (int32_t)vertex_map[t.c];
}

static dim3 post_grid(long long n) { return dim3((unsigned)((n + kPostThreads - 1) / kPostThreads)); }

// nv, nf >= 1, 3 nf <= INT32_MAX (mesh_post_arguments)
static hipError_t mesh_components(const int32_t* faces, int nv, int nf, int32_t* labels, int32_t* sizes, uint32_t* n_out_of_range, void* ws, hipStream_t s) {
    const MeshPostLayout L = mesh_post_layout(nv, nf);
    uint32_t* cursor = at<uint32_t>(ws, L.vert);
    uint2* entries = at<uint2>(ws, L.edge);
    int* parent = at<int>(ws, L.parent);
    const dim3 block(kPostThreads);
    hipError_t e = hipMemsetAsync(cursor, 0, 4 * (size_t)nv, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(n_out_of_range, 0, 4, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(sizes, 0, 4 * (size_t)nf, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post_degree_kernel, post_grid(nf), block, 0, s, faces, nv, nf, cursor, parent, n_out_of_range);
    e = exclusive_scan_in_place(cursor, (uint32_t)nv, at<uint32_t>(ws, L.chunks), nullptr, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post_fill_kernel, post_grid(nf), block, 0, s, faces, nv, nf, cursor, entries);
    hipLaunchKernelGGL(post_unite_kernel, post_grid(3ll * nf), block, 0, s, faces, nv, nf, cursor, entries, parent);
    hipLaunchKernelGGL(post_labels_kernel, post_grid(nf), block, 0, s, nf, parent, labels, sizes);
    return hipGetLastError();
}

// nv, nf >= 1; counts: device {nv_out, nf_out, n_out_of_range}
static hipError_t mesh_filter_count(const int32_t* faces, int nv, int nf, const int32_t* labels, const int32_t* sizes, const int32_t* threshold, void* ws,
                             uint32_t* counts, hipStream_t s) {
    const MeshPostLayout L = mesh_post_layout(nv, nf);
    uint32_t* vertex_map = at<uint32_t>(ws, L.vert);
    uint32_t* face_map = at<uint32_t>(ws, L.edge);
    uint32_t* chunks = at<uint32_t>(ws, L.chunks);
    hipError_t e = hipMemsetAsync(vertex_map, 0, 4 * (size_t)nv, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, 12, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post_flags_kernel, post_grid(nf), dim3(kPostThreads), 0, s, faces, nv, nf, labels, sizes, threshold, vertex_map, face_map, counts + 2);
    e = exclusive_scan_in_place(vertex_map, (uint32_t)nv, chunks, counts, s);
    if (e != hipSuccess) return e;
    return exclusive_scan_in_place(face_map, (uint32_t)nf, chunks, counts + 1, s);
}

// after mesh_filter_count on the same faces and workspace, with the counts it left; nv, nf, nv_out >= 1
static hipError_t mesh_filter_emit(const int32_t* faces, int nv, int nf, const float* vertices, const float* colors, void* ws, uint32_t nv_out, uint32_t nf_out,
                            float* vertices_out, float* colors_out, int32_t* faces_out, hipStream_t s) {
    const MeshPostLayout L = mesh_post_layout(nv, nf);
    const uint32_t* vertex_map = at<uint32_t>(ws, L.vert);
    const uint32_t* face_map = at<uint32_t>(ws, L.edge);
    hipLaunchKernelGGL(post_vertices_kernel, post_grid(nv), dim3(kPostThreads), 0, s, vertex_map, nv, nv_out, reinterpret_cast<const uint32_t*>(vertices),
                       reinterpret_cast<const uint32_t*>(colors), reinterpret_cast<uint32_t*>(vertices_out), reinterpret_cast<uint32_t*>(colors_out));
    if (nf_out > 0)
        hipLaunchKernelGGL(post_faces_kernel, post_grid(nf), dim3(kPostThreads), 0, s, faces, nv, nf, face_map, vertex_map, nf_out, faces_out);
    return hipGetLastError();
}

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

// the checks the three sr_mesh_* post-processing calls share; *work = 0 for a mesh without faces or without vertices
static int mesh_post_arguments(const int32_t* faces, int32_t nv, int32_t nf, const void* workspace, size_t workspace_bytes, bool* work) {
    if (nv < 0 || nf < 0) return fail(SR_ERR_INVALID_ARGUMENT, "nv %d / nf %d is negative", nv, nf);
    if (nf > 0x7FFFFFFF / 3) return fail(SR_ERR_UNSUPPORTED, "%d faces: 3 nf does not fit in int32 (process the mesh in parts)", nf);
    *work = nv > 0 && nf > 0;
    if (!*work) return SR_OK;
    if (!faces) return fail(SR_ERR_INVALID_ARGUMENT, "faces is NULL");
    if ((uintptr_t)faces & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "faces is not 4-B aligned");
    return check_workspace(workspace, workspace_bytes, mesh_post_workspace_bytes(nv, nf));
}

extern "C" {

size_t sr_mesh_post_workspace_bytes(int32_t nv, int32_t nf) {
    if (nv < 0 || nf < 0 || nf > 0x7FFFFFFF / 3) return 0;
    return mesh_post_workspace_bytes(nv, nf);
}

int sr_mesh_components(const int32_t* faces, int32_t nv, int32_t nf, int32_t* labels, int32_t* sizes, uint32_t* n_out_of_range, void* workspace,
                       size_t workspace_bytes, void* stream) {
    bool work;
    if (int rc = mesh_post_arguments(faces, nv, nf, workspace, workspace_bytes, &work)) return rc;
    if (!n_out_of_range) return fail(SR_ERR_INVALID_ARGUMENT, "n_out_of_range is NULL");
    if (nf > 0 && nv > 0 && (!labels || !sizes)) return fail(SR_ERR_INVALID_ARGUMENT, "labels / sizes is NULL");
    if (((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)n_out_of_range) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "labels / sizes / n_out_of_range is not 4-B aligned");
    if (nf == 0) return SR_OK;      // no face: nothing to label, nothing out of range, no work
    if (nv == 0) return fail(SR_ERR_INVALID_ARGUMENT, "%d faces without vertices: every index is out of range", nf);
    SR_HIP(mesh_components(faces, nv, nf, labels, sizes, n_out_of_range, workspace, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_mesh_filter_count(const int32_t* faces, int32_t nv, int32_t nf, const int32_t* labels, const int32_t* sizes, const int32_t* threshold,
                         void* workspace, size_t workspace_bytes, uint32_t* counts, void* stream) {
    bool work;
    if (int rc = mesh_post_arguments(faces, nv, nf, workspace, workspace_bytes, &work)) return rc;
    if (!counts) return fail(SR_ERR_INVALID_ARGUMENT, "counts is NULL");
    if ((uintptr_t)counts & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "counts is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) { SR_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), s)); return SR_OK; }
    if (!labels || !sizes) return fail(SR_ERR_INVALID_ARGUMENT, "labels / sizes is NULL");
    if (!threshold) return fail(SR_ERR_INVALID_ARGUMENT, "threshold is NULL");
    if (((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)threshold) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "labels / sizes / threshold is not 4-B aligned");
    SR_HIP(mesh_filter_count(faces, nv, nf, labels, sizes, threshold, workspace, counts, s));
    return SR_OK;
}

int sr_mesh_filter_emit(const int32_t* faces, int32_t nv, int32_t nf, const float* vertices, const float* colors, void* workspace,
                        size_t workspace_bytes, int32_t nv_out, int32_t nf_out, float* vertices_out, float* colors_out, int32_t* faces_out, void* stream) {
    bool work;
    if (int rc = mesh_post_arguments(faces, nv, nf, workspace, workspace_bytes, &work)) return rc;
    if (nv_out < 0 || nf_out < 0) return fail(SR_ERR_INVALID_ARGUMENT, "nv_out %d / nf_out %d is negative", nv_out, nf_out);
    if (nv_out > nv || nf_out > nf) return fail(SR_ERR_INVALID_ARGUMENT, "nv_out %d / nf_out %d: more than the %d vertices / %d faces that came in", nv_out, nf_out, nv, nf);
    if (nf_out > 0 && nv_out == 0) return fail(SR_ERR_INVALID_ARGUMENT, "%d faces without vertices", nf_out);
    if (nv_out > 0 && (!vertices || !vertices_out)) return fail(SR_ERR_INVALID_ARGUMENT, "vertices / vertices_out is NULL");
    if (nv_out > 0 && colors && !colors_out) return fail(SR_ERR_INVALID_ARGUMENT, "colors_out is NULL (colors is given)");
    if (nf_out > 0 && !faces_out) return fail(SR_ERR_INVALID_ARGUMENT, "faces_out is NULL");
    if (((uintptr_t)vertices | (uintptr_t)colors | (uintptr_t)vertices_out | (uintptr_t)colors_out | (uintptr_t)faces_out) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "vertices / colors / vertices_out / colors_out / faces_out is not 4-B aligned");
    if (!work || nv_out == 0) return SR_OK;
    SR_HIP(mesh_filter_emit(faces, nv, nf, vertices, colors, workspace, (uint32_t)nv_out, (uint32_t)nf_out, vertices_out, colors_out, faces_out,
                            static_cast<hipStream_t>(stream)));
    return SR_OK;
}

}  // extern "C"
