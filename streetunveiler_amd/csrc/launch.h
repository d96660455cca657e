// launch.h -- everything that crosses translation units on the host side: the launchers, their scratch sizes and the host-only types
// they take.  Each is declared here exactly once; api.hip and every file that defines or calls one of them includes this header, so a
// changed parameter list is a compile error where it is defined, not an unresolved symbol when the library is loaded.
// Host-only: nothing in here is a kernel parameter except PostCam, LossImages, CeArgs, SurfaceRegArgs, SkyWeights, DensifyRule, the three Tsdf
// structs, the two Mesh structs and the two Unveil structs, which their kernels take by value.
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

// ---- knn.hip -------------------------------------------------------------------------------------------------------------------------
size_t knn_workspace_bytes(int nq, int nr);
hipError_t knn_mean_dist2(int nq, const float* query, int nr, const float* reference, int K, int take_sqrt, float* out, void* ws,
                          size_t ws_bytes, RankMode rank_mode, hipStream_t s);
// The kNN's ordering of a cloud, step by step, for cluster.hip: bounds -> Morton codes, sort, sorted (x, y, z, index) array -> the AABB
// of every run of kKnnBox curve-consecutive points.  `masked`: a point with active[i] == 0 (active == nullptr: none) or a non-finite
// coordinate is left out of the bounds and the boxes, sorted behind every other point and stored as (inf, inf, inf).
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

// ---- cluster.hip ---------------------------------------------------------------------------------------------------------------------
size_t cluster_workspace_bytes(int n);
hipError_t cluster_radius(int n, const float* xyz, const uint8_t* active, float radius, int64_t* labels, void* ws, size_t ws_bytes,
                          RankMode rank_mode, hipStream_t s);

// ---- postprocess.hip -----------------------------------------------------------------------------------------------------------------
struct PostCam {
    int W, H;
    float fx, fy, depth_ratio;
    const float* view;   // device [16] world_view_transform (W2C^T, row-major)
};
hipError_t launch_postprocess_forward(const PostCam& cam, const float* allmap, float* rend_normal, float* surf_depth,
                                      float* surf_normal, float* surf_point, hipStream_t s);
hipError_t launch_postprocess_backward(const PostCam& cam, const float* allmap, const float* g_rend_normal, const float* g_surf_depth,
                                       const float* g_surf_normal, const float* g_surf_point, float* scratch6, float* g_allmap,
                                       hipStream_t s);

// ---- image_loss.hip ------------------------------------------------------------------------------------------------------------------
struct LossImages {
    int W, H, C;
    float lambda;
    const float* image;   // [C,H,W]
    const float* gt;      // [C,H,W]
    const float* sky;     // [C,H,W] or NULL
    const float* alpha;   // [1,H,W] or NULL (with sky)
};
bool image_loss_supported(int W, int H, int C);
size_t image_loss_partial_bytes();
hipError_t launch_image_loss_forward(const LossImages& a, void* workspace, float* out3, hipStream_t s);
hipError_t launch_image_loss_backward(const LossImages& a, const void* workspace, const float* g_loss, float* g_image, float* g_sky,
                                      float* g_alpha, hipStream_t s);

// ---- aux_loss.hip --------------------------------------------------------------------------------------------------------------------
constexpr int kCeMaxClasses = 8;
enum class CeTarget { kProbabilities = 0, kLabelsU8 = 1, kLabelsI32 = 4, kLabelsI64 = 8 };   // the labels' values are their widths in bytes
struct CeArgs {            // a kernel parameter, by value: the class weights travel in the launch
    int C;
    size_t N;              // H * W
    float w[kCeMaxClasses];
    const float* x;        // [C,H,W] logits
    const void* target;    // [H,W] labels or [C,H,W] float probabilities
};
struct SurfaceRegArgs {    // a kernel parameter, by value
    size_t N;
    double lambda_normal, lambda_dist;
    const float* rend_normal;   // [3,H,W]
    const float* surf_normal;   // [3,H,W]
    const float* rend_dist;     // [1,H,W]
};
bool aux_loss_supported(size_t n);              // the element counts the launches below can address
size_t aux_loss_workspace_bytes(size_t n);      // per-block partial sums of n pixels / Gaussians
hipError_t launch_semantic_ce_forward(const CeArgs& a, CeTarget form, void* workspace, float* out1, hipStream_t s);
hipError_t launch_semantic_ce_backward(const CeArgs& a, CeTarget form, const float* g_loss, float* g_x, hipStream_t s);
hipError_t launch_surface_reg_forward(const SurfaceRegArgs& a, void* workspace, float* out3, hipStream_t s);
// a NULL gradient pointer is skipped
hipError_t launch_surface_reg_backward(const SurfaceRegArgs& a, const float* g_loss, float* g_rend_normal, float* g_surf_normal, float* g_rend_dist,
                                       hipStream_t s);
hipError_t launch_opacity_shrink_forward(size_t P, const float* opacity, bool activated, void* workspace, float* out1, hipStream_t s);
hipError_t launch_opacity_shrink_backward(size_t P, const float* opacity, bool activated, const float* g_loss, float* g_opacity, hipStream_t s);

// ---- sky.hip -------------------------------------------------------------------------------------------------------------------------
constexpr int kSkyParams = 64 * 16 + 64 + 2 * (64 * 64 + 64) + 3 * 64 + 3;   // 9603: {W0sh c W1 b1 W2 b2 W3 b3}
constexpr int kSkyParamsPadded = kSkyParams + 1;
constexpr int kSkyDefaultForwardGroups = 1024;    // workgroups of 256 pixels where max_workgroups == 0: a few per CU
constexpr int kSkyDefaultBackwardGroups = 256;    // one per CU: its sums, weights and panels take most of a CU's LDS
struct SkyWeights {        // a kernel parameter, by value: device pointers
    const float *w0sh, *c, *w1, *b1, *w2, *b2, *w3, *b3;
};
int sky_backward_groups(int max_workgroups);
size_t sky_workspace_bytes(int max_workgroups);   // the float64 parameter-gradient set of every workgroup of the backward
hipError_t launch_sky_forward(int W, int H, const float* cam, const SkyWeights& p, int max_workgroups, float* out, hipStream_t s);
// grads: g_w0sh, g_c, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3; a NULL pointer is skipped
hipError_t launch_sky_backward(int W, int H, const float* cam, const SkyWeights& p, const float* g_out, int max_workgroups, void* workspace,
                               float* const (&grads)[8], hipStream_t s);

// ---- optimizer.hip -------------------------------------------------------------------------------------------------------------------
bool adam_supported(const SrAdamSegment* segments, int n_segments);
hipError_t launch_adam_step(const SrAdamSegment* segments, int n_segments, double beta1, double beta2, double eps, hipStream_t s);
bool adam_rows_supported(const SrAdamRowSegment* segments, int n_segments);
hipError_t launch_adam_step_rows(const SrAdamRowSegment* segments, int n_segments, const uint8_t* mask, double beta1, double beta2, double eps,
                                 hipStream_t s);
hipError_t launch_densification_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum, float* denom,
                                      float* max_radii2D, hipStream_t s);

// ---- mask_model.hip ------------------------------------------------------------------------------------------------------------------
bool mask_model_supported(int P, int sh_coeffs);
// a NULL output / gradient pointer is skipped; a delta whose SR_MASK_FIXED_* bit is set is not read
hipError_t launch_mask_compose(int P, int sh_coeffs, const SrMaskTensors& base, const SrMaskTensors& delta, const uint8_t* mask,
                               uint32_t fixed_bits, const SrMaskEffective& out, hipStream_t s);
hipError_t launch_mask_compose_backward(int P, int sh_coeffs, const SrMaskEffective& upstream, const uint8_t* mask, const SrMaskTensors& d_delta,
                                        hipStream_t s);

// ---- densify.hip ---------------------------------------------------------------------------------------------------------------------
struct DensifyRule {   // a kernel parameter, by value
    float max_grad, min_opacity, percent_dense_extent, ws_limit;   // ws_limit < 0: no world-size test
    int select;        // 0: nothing is clone- or split-selected and accum / denom are not read (max_grad is +inf or NaN)
};
size_t densify_workspace_bytes(int P);
// counts_pinned_dev: the device address of four pinned host words the totals kernel stores K, C, S, H into, or NULL
hipError_t densify_plan(int P, const float* accum, const float* denom, const float* opacity, const float* scaling, const DensifyRule& rule,
                        const uint8_t* prune_mask, void* workspace, uint32_t* counts_pinned_dev, hipStream_t s);
const uint32_t* densify_counts_device(int P, const void* workspace);   // the same four words inside the workspace
hipError_t densify_apply(int P, const uint32_t* counts, const float* noise, const float* rotation, const float* scaling,
                         const SrDensifySegment* segments, int n_segments, const void* workspace, hipStream_t s);

// ---- tsdf.hip ------------------------------------------------------------------------------------------------------------------------
struct TsdfViewsDev {      // kernel parameters, by value
    const float* maps;     // device [V,H,W] depths (channels 1) or [V,H,W,4] (depth, r, g, b) records (channels 4)
    const float* full_proj;   // device [V,16]
    int V, H, W, channels;
};
struct TsdfSpace {
    float trunc;           // (float)(5 * voxel_size)
    int contract;          // 1: the samples are in contracted space (center, radius), the truncation is adaptive
    float center[3], radius;
};
struct TsdfGrid {          // sample (ix, iy, iz) = fmaf(index, step, lo) per axis; thread i is ix - ix0 = i / (ny nz), iy, iz
    float lo[3], step[3];
    int ny, nz, ix0;
};
// grid == nullptr: the n samples are read from `samples` [n,3]; rgb (with channels 4) and weight may be nullptr
hipError_t launch_tsdf_fuse(const TsdfViewsDev& views, const TsdfSpace& space, const TsdfGrid* grid, int n, const float* samples, float* tsdf,
                            float* rgb, float* weight, hipStream_t s);

// ---- mesh.hip ------------------------------------------------------------------------------------------------------------------------
struct MeshGrid {          // kernel parameters, by value
    int nx, ny, nz;        // every axis at least 2 (a grid without cells never reaches a launch)
    uint32_t n;            // nx ny nz < 2^31
    float level;
};
struct MeshFrame {         // grid point (ix, iy, iz) sits at fmaf(index, step, lo) per axis
    float lo[3], step[3];
};
size_t mesh_workspace_bytes(uint32_t n);
// counts: device {Nv, Nf}; a count is 0xFFFFFFFF where Nv or 3 Nf is beyond int32
hipError_t mesh_count(const float* volume, const MeshGrid& g, void* workspace, uint32_t* counts, hipStream_t s);
// after mesh_count on the same volume, level and workspace; space.contract: the vertices are un-contracted and un-normalised
hipError_t mesh_emit(const float* volume, const MeshGrid& g, const MeshFrame& frame, const TsdfSpace& space, void* workspace, uint32_t n_vertices,
                     uint32_t n_faces, float* vertices, int32_t* faces, hipStream_t s);

// ---- mesh_post.hip -------------------------------------------------------------------------------------------------------------------
size_t mesh_post_workspace_bytes(int nv, int nf);
// nv, nf >= 1 and 3 nf <= INT32_MAX in all three.  labels, sizes: device [nf]; n_out_of_range: device [1]
hipError_t mesh_components(const int32_t* faces, int nv, int nf, int32_t* labels, int32_t* sizes, uint32_t* n_out_of_range, void* ws, hipStream_t s);
// threshold: device [1]; counts: device {nv_out, nf_out, n_out_of_range}
hipError_t mesh_filter_count(const int32_t* faces, int nv, int nf, const int32_t* labels, const int32_t* sizes, const int32_t* threshold, void* ws,
                             uint32_t* counts, hipStream_t s);
// after mesh_filter_count on the same faces and workspace, with the counts it left; nv_out >= 1; colors / colors_out may be nullptr
hipError_t mesh_filter_emit(const int32_t* faces, int nv, int nf, const float* vertices, const float* colors, void* ws, uint32_t nv_out, uint32_t nf_out,
                            float* vertices_out, float* colors_out, int32_t* faces_out, hipStream_t s);
// The exclusive scan of n >= 1 words in place (n < 2^31, the sum fits in 32 bits), also unveil.hip's compaction: chunks of
// kScanInPlaceChunk items, `chunks` = scan_in_place_chunk_words(n) words of device scratch; total_out (device, may be nullptr) gets the sum
constexpr int kScanInPlaceChunk = 4096;
inline size_t scan_in_place_chunk_words(uint32_t n) { return ((size_t)n + kScanInPlaceChunk - 1) / kScanInPlaceChunk + 1; }
hipError_t exclusive_scan_in_place(uint32_t* data, uint32_t n, uint32_t* chunks, uint32_t* total_out, hipStream_t s);

// ---- unveil.hip ----------------------------------------------------------------------------------------------------------------------
constexpr int kUnveilCamFloats = 24;   // a camera row: w2c rows 0..2 (12), K (9), max_z (+inf: none), reso_scale (0: none), one unused
constexpr int kDilateRows = 32;        // output rows of a dilation tile (64 columns wide); the tile rows are grid.y: H <= 32 * 65535 (api.hip)
struct UnveilSemantic {    // a kernel parameter, by value: device pointers
    int P, F, Hm, Wm;
    uint32_t remain_bit;   // bits 0..30
    const float* xyz;      // [P,3]
    const float* cams;     // [F,kUnveilCamFloats]
    const int32_t* hw;     // [F,2] = (h, w)
    const uint8_t* maps;   // [F,Hm,Wm] labels
};
struct UnveilConditions {  // a kernel parameter, by value: device pointers; the images are [C,H,W] float32, the outputs [H,W,C] uint8
    int H, W;
    const float *full_render, *full_alpha, *background_render, *background_alpha, *background_depth, *background_normal, *sky;
    uint8_t *original_rgb, *inpainted_rgb, *empty_opacity, *inpainted_depth, *inpainted_normal;
};
size_t unveil_workspace_bytes(int P, int F);
// P >= 1 in all four.  count == nullptr: the mask alone; else the admitted points' offsets stay in the workspace and *count (device) = n
hipError_t points_in_frame(int P, const float* xyz, const float* cam, const int32_t* hw, uint8_t* mask, void* ws, uint32_t* count, hipStream_t s);
hipError_t points_in_frame_emit(int P, const float* xyz, const float* cam, const int32_t* hw, const void* ws, uint32_t n, int64_t* pix, float* depth,
                                hipStream_t s);
hipError_t frame_visibility(int P, int F, const float* xyz, const float* cams, const int32_t* hw, void* ws, int64_t* count, double* depth_sum,
                            hipStream_t s);
hipError_t semantic_mask_of_points(const UnveilSemantic& a, uint8_t* mask, uint64_t* n_out_of_range, hipStream_t s);
// H, W >= 1, H W < 2^31, H <= kDilateRows * 65535, W <= INT32_MAX - 128, 1 <= k <= 31 in all four; masks and outputs are bytes [H,W]
hipError_t dilate_mask(int H, int W, int k, const uint8_t* mask, uint8_t* out, hipStream_t s);
hipError_t instance_pixel_mask(int H, int W, int k, const float* alpha_a, const float* alpha_b, float threshold, uint8_t* out, hipStream_t s);
hipError_t refill_mask(int H, int W, int C, int k, const float* render_a, const float* render_b, const uint8_t* mask, float eps, uint8_t* out,
                       hipStream_t s);
hipError_t inpaint_conditions(const UnveilConditions& a, float threshold, int k, uint8_t* mask_out, hipStream_t s);

// ---- voxel.hip -----------------------------------------------------------------------------------------------------------------------
constexpr int kVoxelHeavy = 128;       // a voxel of more members than this gets a wave instead of a lane
constexpr long long kVoxelMaxOffset = 1ll << 21;   // offset^3 must stay inside int64
size_t voxel_workspace_bytes(uint32_t n);
// n >= 1 in all three; points / colors / normals are [n,3] float32 or float64 (the *_f64 flags).  bounds: device [7] doubles = min xyz, max
// xyz over the finite rows, the number of non-finite rows
hipError_t voxel_bounds(uint32_t n, const void* points, int points_f64, void* ws, double* bounds, hipStream_t s);
// labels: nullptr or [n] int32 / int64 (label_bytes 4 / 8); lo: three host doubles; 1 <= offset < kVoxelMaxOffset; counts (device, may be
// nullptr): {voxels, kept, bad labels}
hipError_t voxel_group(uint32_t n, const void* points, int points_f64, const void* labels, int label_bytes, const double* lo, double voxel_size,
                       long long offset, void* ws, uint32_t* counts, RankMode rank_mode, hipStream_t s);
// after voxel_group on the same points and workspace; rows >= 1: the kept count read back.  A nullptr attribute or output is skipped
hipError_t voxel_emit(uint32_t n, const void* points, int points_f64, const void* colors, int colors_f64, const void* normals, int normals_f64,
                      const void* ws, uint32_t n_voxels, uint32_t rows, float* out_points, float* out_colors, float* out_normals, int32_t* out_labels,
                      int32_t* out_counts, int64_t* out_index, hipStream_t s);

// ---- lidar_label.hip -----------------------------------------------------------------------------------------------------------------
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
size_t lidar_label_workspace_bytes(uint64_t rows);
// n >= 1 in all three; counts: device [2] uint64
hipError_t lidar_label_decide(const LabelCloud& c, const SrLabelView* views, int cameras, int check_range, bool mirrored, const uint8_t* lut, void* ws,
                              uint64_t* counts, hipStream_t s);
hipError_t lidar_vote(const LabelCloud& c, const SrLabelView* views, int n_views, int n_classes, const uint8_t* lut, void* ws, uint8_t* valid_mask,
                      uint64_t* counts, hipStream_t s);
hipError_t lidar_label_emit(const LabelCloud& c, const void* ws, uint32_t n_rows, void* out_xyz, double* out_rgb, int32_t* out_semantics, int64_t* out_index,
                            int32_t* rows_per_sweep, hipStream_t s);

}  // namespace sr
