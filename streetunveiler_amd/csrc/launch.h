// launch.h -- what crosses kernel files on the host side: the launchers of the rasteriser's stages (preprocess, sort, binning, blend, class
// passes), which api.hip sequences, and the few host-only types and steps that more than one kernel file uses -- the blend choice, the
// workspace carver, the kNN's ordering of a cloud (knn.hip, cluster.hip), TsdfSpace (tsdf.hip, mesh.hip, contraction.h) and the in-place
// exclusive scan (mesh_post.hip, unveil.hip, voxel.hip, lidar_label.hip).  Each is declared here exactly once and every file that defines
// or calls one includes this header, so a changed parameter list is a compile error where it is defined, not an unresolved symbol when the
// library is loaded.  A launcher or kernel-parameter struct that one file alone uses lives in that file; what the files with C entry points
// share beyond this is in abi.h.  Of the types here only TsdfSpace is a kernel parameter.
#pragma once
#include "common.h"


namespace sr {

// ---- the blend pair of a frame (api.hip choose_blend decides, once per call; the launchers switch on it) -----------------------------
// The forward kernels of the 16x16 tile with three colour channels (every other shape / channel count has one kernel, plus the counting
// variant of 16x16 with three or six channels).
enum class ForwardBlend {
    kDevicePicked,     // render_forward_auto_kernel: rows or quadrant bands per frame, from the emission scan's counts
    kQuadrantBands,    // render_forward_kernel<false, 3, 2, 1, 2>
    kRows,             // render_forward_rows_kernel<2, 1, 2>
    kRowsCellMasks,    // render_forward_rows_kernel<2, 1, 2, true>: hit masks per 4x4 cell, for BackwardBlend::kRows
    kCoop,             // render_forward_coop_kernel
    kCounting,         // render_forward_kernel<true, NCH, 2, 2, 1> (SrFrame.blend_counters)
};
enum class BackwardBlend {
    kByTileCount,      // the cooperative kernel below kCoopBelowTiles tiles, else one wave per tile (render_bwd.hip)
    kOneWave,          // render_backward_kernel
    kCoop,             // render_backward_coop_kernel<3>
    kRows,             // render_backward_rows_kernel: reads CELL-granular hit masks
};
enum class HitMaskFormat { kQuadrant, kCell };   // what the forward writes per list entry and the backward of the same frame reads
struct BlendChoice {
    ForwardBlend forward;
    BackwardBlend backward;
    HitMaskFormat mask;
    bool cull;   // quadrant culling on (SR_FLAG_NO_QUADRANT_CULL clear)
};

// ---- workspace carving ---------------------------------------------------------------------------------------------------------------
// A layout = the byte offsets of a buffer's regions, every region 256-B aligned, + its total: one Carver walk per layout function, so a
// size and the pointers into it cannot drift apart.  A zero-byte region takes no room (callers that rely on distinct regions clamp their
// counts to 1).  at<T>: the typed pointer of a region.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};
template <class T> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// ---- preprocess.hip ------------------------------------------------------------------------------------------------------------------
hipError_t launch_preprocess_forward(int P, const FrameDev& f, const SrGaussians& g, float4* recs, uint32_t* depth_keys,
                                     uint32_t* tiles_touched, uint2* rect, uint8_t* clamped, int32_t* radii, hipStream_t s);
hipError_t launch_preprocess_backward(int P, const FrameDev& f, const SrGaussians& g, const int32_t* radii,
                                      const uint8_t* clamped, const float4* recs, const float4* inst_grads, const uint8_t* written,
                                      const uint32_t* tiles_touched, const SrGradients& out, hipStream_t s);
hipError_t launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s);
hipError_t launch_sh_gradient_expand(int P, int M, int deg, int V, const float* means3D, const float* campos, const float* gc,
                                     float* dL_dsh, hipStream_t s);
hipError_t launch_color_gradients(int P, const FrameDev& f, const int32_t* radii, const uint8_t* clamped, const float4* recs, const float4* inst_grads,
                                  const uint8_t* written, const uint32_t* tiles_touched, bool mask_clamped, float* dL_dcolors, hipStream_t s);

// ---- radix_sort.hip ------------------------------------------------------------------------------------------------------------------
size_t radix_sort_temp_bytes(uint32_t n);
// `one_sweep`: SR_FLAG_ONE_SWEEP_SORT -- the one-sweep passes where they apply (32-bit keys, from kOneSweepFrom items up)
hipError_t radix_sort_pairs(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t n,
                            int total_bits, void* temp, size_t temp_bytes, hipStream_t s, const uint2* aux_src, uint2* aux_out, RankMode rank_mode,
                            bool one_sweep, int rect_bx = 0, int rect_by = 0, const uint32_t* n_live = nullptr);
// exclusive scan of `rows` histogram rows of `stride` words in place (a block per row) + the row totals; a row ends with the blocks of
// items_per_block items that hold the min(*n_dev, n_host) items (n_dev == nullptr: n_host)
hipError_t launch_scan_rows(int rows, uint32_t* hist, int stride, uint32_t n_host, const uint32_t* n_dev, int items_per_block, uint32_t* row_total,
                            hipStream_t s);
size_t tile_count_scan_temp_bytes(uint32_t n);
hipError_t tile_count_scan(const uint32_t* counts, uint32_t* out, uint32_t n, void* temp, size_t temp_bytes, uint32_t* total_host, hipStream_t s);
hipError_t launch_rank_selfcheck(uint32_t* result, hipStream_t s);
hipError_t lds_atomic_ranks(const uint32_t* digits, uint32_t* ranks, uint32_t n, int bins, hipStream_t s);

// ---- binning.hip ---------------------------------------------------------------------------------------------------------------------
size_t depth_sort_temp_bytes(int P);
size_t tile_scan_temp_bytes(int P);
size_t expand_x_hist_bytes(int P, int tiles_x);
size_t expand_y_hist_bytes(uint32_t D, int tiles_y);
hipError_t run_depth_sort(int P, const uint32_t* depth_keys, const uint2* rect, uint32_t* sorted_keys,
                          uint32_t* sorted_gid, uint2* rect_sorted, void* temp, size_t temp_bytes, RankMode rank_mode, bool one_sweep, int tiles_x,
                          int tiles_y, const uint32_t* n_visible, hipStream_t s);
hipError_t run_tile_count_scan(int P, const uint32_t* tiles_touched, uint32_t* first, void* block_base, size_t base_bytes, uint32_t* total_host,
                               hipStream_t s);
hipError_t run_expand_columns(int P, int tiles_x, int n_tiles, const uint2* rect_sorted, const uint32_t* sorted_gid, uint2* columns,
                              uint32_t* n_columns, uint32_t* hist, uint32_t* row_total, uint32_t* tile_counts, RankMode rank_mode, const uint32_t* n_visible,
                              hipStream_t s);
hipError_t run_expand_rows(uint32_t D, int tiles_x, int tiles_y, const uint2* columns, const uint32_t* n_columns, uint32_t* hist, uint32_t* row_total,
                           uint32_t* point_list, uint32_t* tile_counts, RankMode rank_mode, hipStream_t s);
hipError_t run_tile_ranges_order(int n_tiles, const uint32_t* tile_counts, uint2* ranges, uint32_t* order, hipStream_t s);
hipError_t run_capacity_guard(uint32_t* counts, uint32_t capacity, hipStream_t s);
hipError_t launch_zero_bytes(void* p, size_t n, hipStream_t s);

// ---- render.hip, render_bwd.hip ------------------------------------------------------------------------------------------------------
hipError_t launch_render_forward(const FrameDev& f, const uint2* ranges, const uint32_t* tile_order, const uint32_t* point_list, const float4* recs,
                                 const float* extra, float* out_color, float* out_allmap, float* final_T, uint32_t* n_contrib, uint16_t* hit_mask,
                                 const BlendChoice& blend, unsigned long long* counters, const uint32_t* frame_counts, hipStream_t s);
hipError_t launch_render_backward(const FrameDev& f, const uint2* ranges, const uint32_t* tile_order, const uint32_t* point_list, const float4* recs,
                                  const float* extra, const float* final_T, const uint32_t* n_contrib, const float* dL_dcolor,
                                  const float* dL_dallmap, const uint16_t* hit_mask, float4* inst_grads, uint8_t* written, bool precomp_color_grads,
                                  BackwardBlend blend, hipStream_t s);
hipError_t launch_pair_decisions(const FrameDev& f, const uint2* ranges, const uint32_t* point_list, const float4* recs,
                                 unsigned long long* valid_bits, unsigned long long* use3d_bits, hipStream_t s);

// ---- render_class.hip ----------------------------------------------------------------------------------------------------------------
hipError_t launch_class_partition(int P, int n_tiles, int n_classes, const float* class_cols, const int32_t* class_i32, const uint2* ranges,
                                  const uint32_t* point_list, uint8_t* ids, uint32_t* cls_list, uint2* cls_ranges, hipStream_t s);
hipError_t launch_class_forward(const FrameDev& f, int n_classes, const uint2* cls_ranges, const uint32_t* tile_order, const uint32_t* cls_list,
                                const float4* recs, float* out_dist, float* cls_state, uint32_t* cls_last, uint32_t* tile_total, uint16_t* hit_mask,
                                int cull, hipStream_t s);
// `shared_rec_quads`: 0 = this pass owns the gradient records; else the float4s per record of the colour pass whose records it adds to
hipError_t launch_class_backward(const FrameDev& f, int n_classes, const uint2* cls_ranges, const uint32_t* tile_order, const uint32_t* cls_list,
                                 const float4* recs, const float* cls_state, const uint32_t* cls_last, const uint32_t* tile_total,
                                 const float* dL_ddist, const uint16_t* hit_mask, float4* inst_grads, uint8_t* written, int shared_rec_quads, hipStream_t s);

// ---- knn.hip: the kNN's ordering of a cloud, step by step, also for cluster.hip ---------------------------------------------------------
// bounds -> Morton codes, sort, sorted (x, y, z, index) array -> the AABB of every run of kKnnBox curve-consecutive points.  `masked`: a
// point with active[i] == 0 (active == nullptr: none) or a non-finite coordinate is left out of the bounds and the boxes, sorted behind
// every other point and stored as (inf, inf, inf).
constexpr int kKnnBox = 512;
struct CloudOrder {   // device arrays of n entries each
    uint32_t* codes;
    uint32_t* codes_sorted;
    uint32_t* order;
    float4* sorted;
};
size_t cloud_bounds_partial_bytes(int n);
hipError_t cloud_bounds_masked(const float* pts, const uint8_t* active, int n, float* partial, float* bounds, hipStream_t s);
hipError_t cloud_order(const float* pts, const uint8_t* active, bool masked, int n, const float* bounds, const CloudOrder& o, void* sort_temp,
                       size_t temp_bytes, RankMode rank_mode, hipStream_t s);
hipError_t cloud_boxes(const float4* sorted, int n, float4* boxes, hipStream_t s);

// ---- tsdf.hip, mesh.hip, contraction.h -----------------------------------------------------------------------------------------------
struct TsdfSpace {
    float trunc;           // (float)(5 * voxel_size)
    int contract;          // 1: the samples are in contracted space (center, radius), the truncation is adaptive
    float center[3], radius;
};

// ---- mesh_post.hip: also the compaction of unveil.hip, voxel.hip and lidar_label.hip ---------------------------------------------------
// The exclusive scan of n >= 1 words in place (n < 2^31, the sum fits in 32 bits): chunks of kScanInPlaceChunk items, `chunks` =
// scan_in_place_chunk_words(n) words of device scratch; total_out (device, may be nullptr) gets the sum
constexpr int kScanInPlaceChunk = 4096;
inline size_t scan_in_place_chunk_words(uint32_t n) { return ((size_t)n + kScanInPlaceChunk - 1) / kScanInPlaceChunk + 1; }
hipError_t exclusive_scan_in_place(uint32_t* data, uint32_t n, uint32_t* chunks, uint32_t* total_out, hipStream_t s);

}  // namespace sr
