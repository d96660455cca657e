/*
 * surfel_raster.h -- C-ABI of the MI355X-native 2D-Gaussian (surfel) splatting rasterizer.
 *
 * This is the drop-in boundary for the ONE hot path of StreetUnveiler:
 *     gaussian_renderer.render -> diff_surfel_rasterization.GaussianRasterizer
 *         -> _C.rasterize_gaussians / _C.rasterize_gaussians_backward / _C.mark_visible
 * The reference binds that path through a torch C++ extension (`diff_surfel_rasterization._C`,
 * an un-vendored submodule: /root/reference/.gitmodules:9-12; only importer:
 * /root/reference/gaussian_renderer/__init__.py:11).  The entry points below are what that
 * extension's three functions bind to in this build; the python shim that reproduces the `_C`
 * call shape on top of them is diff_surfel_rasterization/__init__.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every `const float*` / buffer argument is a DEVICE pointer owned by the caller (a torch
 *     tensor kept alive by the autograd ctx) unless the name ends in `_host`.
 *   - the library allocates nothing persistent; all scratch lives in the three caller-owned state
 *     buffers (geom / binning / image) whose sizes come from the sr_*_bytes() queries -- the
 *     counterpart of the reference's resize-callback buffers geomBuffer / binningBuffer / imgBuffer
 *     (call shape: SURVEY.md 8b "Native signatures").
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - return value: 0 on success, negative SrStatus on failure; sr_last_error() gives the text of
 *     the last failure on the calling thread.  No exceptions cross the ABI.
 *   - tensor layouts are the operator's: float32, contiguous; means3D[P,3], opacities[P,1],
 *     scales[P,2], rotations[P,4] (r,x,y,z), shs[P,M,3] (coefficient-major), colors_precomp[P,NC],
 *     transMat_precomp[P,9]; images are planar [C,H,W].  NC = SrGaussians.color_channels: 3 as in the reference, 9 (see the
 *     struct), or 6
 *     (precomputed colours only) = two 3-channel passes over the same geometry folded into one -- what the reference's
 *     render_semantic does with two rasterizer calls (/root/reference/gaussian_renderer/__init__.py:386-431)
 *     (/root/reference/gaussian_renderer/__init__.py:56-138; allmap channel order :149-165).
 */
#ifndef SURFEL_RASTER_H
#define SURFEL_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_ABI_VERSION 10
#define SR_TILE 16            /* default 16x16 pixel tiles (upstream BLOCK_X/BLOCK_Y); see SrFrame.tile_width */
#define SR_SPLAT_FLOATS 20    /* floats per packed splat record (80 B) */
#define SR_GRAD_FLOATS 24     /* floats per gradient record (96 B) */
#define SR_MAX_TILES_PER_AXIS 1024 /* tiles per image axis the binning handles (10-bit row / column fields of the expanding partition):
                                    * frames up to 16384 px per axis with the 16x16 tile, 8192 px with 8x8, 32768 px wide with 32x16;
                                    * larger frames are refused with SR_ERR_INVALID_ARGUMENT (pick a larger tile) */

/* SrGaussians.activations == the GaussianModel activations
 * (/root/reference/scene/gaussian_model.py:63-75, getters :101-123) */
#define SR_ACT_EXP_SCALES 1          /* scales = exp(raw) */
#define SR_ACT_SIGMOID_OPACITY 2     /* opacities = sigmoid(raw) */
#define SR_ACT_NORMALIZE_ROTATIONS 4 /* rotations = raw / max(|raw|, 1e-12) */

typedef enum SrStatus {
    SR_OK = 0,
    SR_ERR_INVALID_ARGUMENT = -1, /* NULL where a pointer is required, bad sizes, both/neither of an exclusive pair */
    SR_ERR_HIP = -2,              /* a HIP runtime call or kernel launch failed */
    SR_ERR_BUFFER_TOO_SMALL = -3, /* a state buffer is smaller than sr_*_bytes() reports */
    SR_ERR_UNSUPPORTED = -4       /* e.g. sh_degree > 3 */
} SrStatus;

/* Per-call camera / raster settings == GaussianRasterizationSettings
 * (/root/reference/gaussian_renderer/__init__.py:39-52). */
typedef struct SrFrame {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;     /* active degree (0..3) */
    int32_t prefiltered;   /* always 0 at the reference's call sites; accepted, ignored */
    int32_t debug;         /* 1: synchronise + check after every kernel */
    const float* bg;          /* device [NC] (3, or 6 with SrGaussians.color_channels == 6) */
    const float* viewmatrix;  /* device [16] = world_view_transform (W2C^T), row-major */
    const float* projmatrix;  /* device [16] = full_proj_transform ((P*W2C)^T), row-major */
    const float* campos;      /* device [3] */
    int32_t tile_width;       /* 0 = 16 (the reference's BLOCK_X); BASELINE config 5 sweeps 8x8, 16x8, 16x16, 32x8, 32x16.  The 6- and
                               * 9-channel passes (SrGaussians.color_channels) and the per-class pass exist for every shape, the counter
                               * variant (blend_counters) for 16x16 only */
    int32_t tile_height;      /* 0 = 16 (BLOCK_Y).  Same shape in every call that shares the state buffers */
    uint32_t flags;           /* SR_FLAG_* bits; per call, nothing about a call is process-wide state */
    uint64_t* blend_counters; /* NULL, or device [16] u64 owned by the caller: selects the COUNTING variant of the forward blend (same
                               * results, slow), which adds to [0] list entries staged, [1] entries kept by the quadrant culling,
                               * [2] (entry, quadrant) tests run, [3] tests with >= 1 contributing pixel, [4] contributing (pixel, entry)
                               * pairs, [5] / [6] tests with a contributing pixel in rows 0-3 / rows 4-7 of the quadrant, [7] entries with a
                               * contributing pixel anywhere in the tile (= the gradient records the backward writes), [8] (entry, 4x4 cell) pairs
                               * with a contributing pixel, [9] the wave steps a 16-lane-row mapping would take (sum over rounds of 64
                               * entries and quadrants of the busiest cell's pair count), [10] / [11] the same two counting the pairs the row-mapped
                               * forward's cell culling at staging keeps (hits and misses; the slab-extent test), [12] / [13] unused (zero), [14] exact
                               * (entry, cell) hits that culling would DROP (must be 0), [15] the pairs of [10] as an octagon-vs-cell test keeps them.  16x16 tile with
                               * 3 or 6 colour channels; any other request returns SR_ERR_UNSUPPORTED (never silent zeros) */
} SrFrame;
#define SR_FLAG_NO_QUADRANT_CULL 1u  /* forward blend: run every list entry against every 8x8 quadrant instead of dropping entries that
                                      * provably cannot reach alpha >= 1/255 there.  Results are bit-identical either way (a test
                                      * requires it); the switch exists for that test and for A/B timing */
#define SR_FLAG_BALLOT_RANKING 2u    /* binning: rank the items of a wave with match-any ballots instead of LDS-atomic return values.  The
                                      * atomic path relies on gfx950 returning ds_add_rtn_u32 results in lane order (undocumented), so
                                      * the library checks that property on every device before its first sort (sr_rank_mode) and falls
                                      * back to the ballots by itself; this flag forces the fallback for one call (tests, A/B timing).
                                      * The lists are bit-identical either way */
#define SR_FLAG_ROW_MAPPED_FORWARD 4u /* forward blend, 16x16 tile with three colour channels: force the row-mapped kernel (the four 16-lane rows
                                      * of a wave are the four 4x4 cells of a quadrant, every row walks its own list of entries) ... */
#define SR_FLAG_QUADRANT_MAPPED_FORWARD 8u /* ... or the quadrant-mapped one (one entry on all 64 lanes).  Bit-identical images, state and hit
                                      * masks (a test requires it).  Without either flag the DEVICE picks per frame from the duplicates per
                                      * visible Gaussian the emission scan leaves in the geometry state: rows below 6.5 (small footprints:
                                      * -3 % at 1920x1080 / 3 M, -11 % at 1280x720), quadrants above (+10 % for the rows at 3840x2160):
                                      * DESIGN.md 4.  The flags exist for the A/B and the test.  SR_FLAG_ROW_MAPPED_FORWARD with any other
                                      * tile shape / channel count / blend_counters / SR_FLAG_NO_QUADRANT_CULL: SR_ERR_UNSUPPORTED */

#define SR_FLAG_FORWARD_ONLY 16u      /* no backward will follow this forward (the reference's inference callers run the operator under
                                      * torch.no_grad(): /root/reference/render.py:68, /root/reference/utils/mesh_utils.py:82-100): K1 does not
                                      * compute or write the 36-B/Gaussian SH direction Jacobian, K6 does not write the backward's state
                                      * (final_T / M1 / M2, last and median contributor: 20 B/pixel; the 2-B/duplicate hit masks).  Set in
                                      * BOTH sr_forward_plan and sr_forward_render; `image` may then be NULL / 0 bytes.  out_color, out_allmap
                                      * and radii are bit-identical to the training forward (a test requires it); calling a backward on the
                                      * state of such a forward is undefined */

#define SR_FLAG_NO_PRECOMP_COLOR_GRAD 32u /* backward (sr_backward / sr_backward_blend), 6 / 9 colour channels: the caller does not want dL/dcolors_precomp
                                      * (SrGradients.dL_dcolors NULL) -- the one-hot class channels of render_semantic are constants -- so K7 does not
                                      * form those sums (the channels still feed dL/dalpha); every other gradient is unchanged */

#define SR_FLAG_BINNING_CAPACITY 64u  /* the forward WITHOUT its host read-back (round 6).  By default sr_forward_plan waits once for D, the frame's duplicate
                                      * count, because the caller sizes the binning buffer from it -- as the reference does.  With this flag, set in EVERY call of
                                      * the frame (plan, render, backward):
                                      *   - sr_forward_plan queues K1, the scan and the depth sort and returns at once; *num_rendered_host = 0xFFFFFFFF;
                                      *   - `num_rendered` of sr_forward_render / sr_binning_bytes / sr_backward* / sr_backward_workspace_bytes is the CAPACITY (in
                                      *     duplicates) the caller chose for the binning buffer and the workspace -- e.g. 1.25 x the largest D it has seen;
                                      *   - a one-thread guard kernel compares the frame's D with the capacity on the device.  It fits: results bit-identical to
                                      *     the default mode.  It does not: nothing is binned, the images hold the background, every gradient is zero, no kernel reads or
                                      *     writes beyond the buffers, and SrGeomView.frame_counts[2] = 1 -- the caller looks at that word when it next synchronises
                                      *     anyway (frame_counts[0] = the exact D) and renders the frame again with a larger buffer.
                                      * No pinned memory, event or host wait is touched: the whole forward + backward can be captured into a HIP graph.
                                      * Not for the per-class passes (SR_ERR_UNSUPPORTED). */

#define SR_FLAG_ONE_SWEEP_SORT 128u   /* sr_forward_plan / sr_debug_radix_sort: the depth sort's four passes as ONE-SWEEP passes (one up-front digit count, then
                                      * one kernel per pass with decoupled look-back over relaxed-atomic status words: six launches instead of twelve).  Bit-identical
                                      * order; measured SLOWER on MI355X at the benchmark's size (0.190 vs 0.157 ms at 3 M keys: csrc/radix_sort.hip), hence a flag */

#define SR_FLAG_ONE_WAVE_BACKWARD 256u /* both blend kernels, 16x16 tile with three colour channels: force the full-size forms (two band waves per tile forward, one
                                      * wave per tile backward) ... */
#define SR_FLAG_COOP_BACKWARD 512u     /* ... or the cooperative ones (four waves per tile, one per 8x8 quadrant, ONE staging of every entry; backward: one record per
                                      * duplicate as before; forward: images and state bit-identical to the band kernel's -- measured no faster anywhere, so it
                                      * only runs with this flag).  Set in sr_forward_render and in the backward.  Without either
                                      * flag the library picks by the frame's tile count: cooperative below 2 600 tiles of 16x16 (the reference's `-r 4` frames:
                                      * 600 tiles cannot fill the GPU with one wave each), one wave per tile above.  Same tile lists either way; gradients
                                      * agree up to the order of a four-term sum.  The flags exist for the A/B and the tests.
                                      * At most ONE of SR_FLAG_ONE_WAVE_BACKWARD, SR_FLAG_COOP_BACKWARD and SR_FLAG_ROW_BACKWARD per call: sr_forward_render,
                                      * sr_backward_blend, sr_backward_geometry and sr_backward return SR_ERR_INVALID_ARGUMENT for two or three of them.  The
                                      * backward of a frame must carry the same one of them as its forward (or none in both): the library keeps no per-frame
                                      * record of which forward ran, so a mismatch across the two calls is NOT detected */

#define SR_FLAG_ROW_BACKWARD 1024u     /* 16x16 tile, three colour channels, culling on: the ROW-MAPPED blend pair -- the forward (row-mapped kernel) writes its hit masks
                                      * per (entry, 4x4 cell) instead of per (entry, 8x8 quadrant), and the backward's four 16-lane rows each walk their own cell's
                                      * list (render_backward_rows_kernel).  Must be set in sr_forward_render AND in the backward of the same frame (the hit-mask
                                      * format differs).  Images bit-identical; gradients agree with the one-wave kernel's up to the order of additions.
                                      * MEASURED SLOWER (C3: K7 2.55 ms against 1.65: the per-entry sums are scattered into LDS with float atomics, ~100 LDS cycles
                                      * per wave instruction -- csrc/render_bwd.hip): built and kept as the measured answer, picked nowhere.  The backward checks the
                                      * same preconditions as the forward (16x16, three channels, no SR_FLAG_NO_QUADRANT_CULL: else SR_ERR_UNSUPPORTED) and, like it,
                                      * refuses SR_FLAG_ONE_WAVE_BACKWARD / SR_FLAG_COOP_BACKWARD beside this flag */

/* Per-Gaussian inputs == the keyword arguments of GaussianRasterizer.forward
 * (/root/reference/gaussian_renderer/__init__.py:129-138).  Exactly one of shs / colors_precomp
 * and exactly one of (scales, rotations) / transMat_precomp must be non-NULL. */
typedef struct SrGaussians {
    int32_t P;          /* number of Gaussians */
    int32_t sh_coeffs;  /* M = shs.size(1) (16 for max degree 3); 0 with colors_precomp */
    int32_t color_channels; /* NC: 0 or 3 = rgb; 6 = six precomputed channels (shs must be NULL); 9 = rgb from shs PLUS the six
                             * channels of colors_precomp[P,6] (both non-NULL): render + render_semantic as one pass */
    int32_t activations;    /* SR_ACT_* bits: the given arrays are the reference's RAW parameters and the activation is fused
                             * into K1 (and its adjoint into K8: raw gradients out); 0 = activated inputs as in the reference */
    const float* means3D;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* shs;
    const float* colors_precomp;
    const float* transMat_precomp;  /* the reference's `cov3D_precomp` slot carries a [P,9] transMat in 2DGS */
    const uint8_t* mask;            /* optional [P] (torch.bool storage): 0 = leave this Gaussian out, exactly as if the caller had
                                     * boolean-indexed every input (render_with_mask / semantic filters,
                                     * /root/reference/gaussian_renderer/__init__.py:89-105, 190-325) -- without the copies; radii
                                     * and gradients stay full-size, zero where masked out.  NULL = all */
} SrGaussians;

/* Gradient outputs of the backward == return tuple of _C.rasterize_gaussians_backward.
 * Every non-NULL pointer is fully written (zeros for invisible Gaussians); NULL = not wanted. */
typedef struct SrGradients {
    float* dL_dmeans2D;    /* [P,3] densification proxy (x, y, 0) -- what viewspace_points.grad receives */
    float* dL_dcolors;     /* [P,NC] w.r.t. colors_precomp ([P,6] for NC = 9); with shs as the colour source: [P,3] clamp-masked dL/drgb (the SH adjoint's input, see sr_sh_gradient_expand) */
    float* dL_dopacity;    /* [P,1] */
    float* dL_dmeans3D;    /* [P,3] */
    float* dL_dtransMat;   /* [P,9] */
    float* dL_dsh;         /* [P,M,3]; may be NULL with shs given (frame-parallel ranks ship dL_dcolors instead) */
    float* dL_dscales;     /* [P,2] */
    float* dL_drotations;  /* [P,4] */
} SrGradients;

/* Views into the caller-owned state buffers (for tests / debugging; all device pointers). */
typedef struct SrGeomView {
    const float* splats;           /* [P,20] packed record: Tu.xyz Tv.x | Tv.yz Tw.xy | Tw.z xy.x xy.y opacity | n.xyz r | g b view-depth radius.  Rows with radii == 0 are UNDEFINED: K1 does not write the
                                    * 128-B lines of the record array whose rows are all culled (round 5), so such rows hold whatever the caller's buffer held -- possibly
                                    * NaN; read a row only where radii > 0 (every kernel reaches the records through the tile lists, which hold visible Gaussians only) */
    const uint32_t* depth_keys;    /* [P] float bits of view-space depth; 0xFFFFFFFF when culled */
    const uint32_t* tiles_touched; /* [P] */
    const uint8_t* clamped;        /* [P] bit c set when SH colour channel c was clamped at 0 */
    const uint32_t* sorted_gid;    /* the frame_counts[1] visible Gaussians' ids in ascending (depth bits, id) order (room for P; culled ones are dropped) */
    const uint32_t* frame_counts;  /* [2] D (= *num_rendered_host of sr_forward_plan) and the number of Gaussians with at least one tile: what
                                    * the forward blend picks its mapping by (SR_FLAG_ROW_MAPPED_FORWARD).  With SR_FLAG_BINNING_CAPACITY: [3] -- after
                                    * sr_forward_render [2] = 1 if D exceeded the capacity (and [1] was zeroed: nothing was rendered), else 0 */
} SrGeomView;

typedef struct SrBinningView {
    const uint32_t* point_list;  /* [D] Gaussian id of every sorted duplicate (tile-major, then depth, then id); the tile of entry j is
                                  * the one whose range contains j (the tile ids themselves are not kept after the partition) */
    const uint32_t* ranges;      /* [tiles,2] (begin, end) into point_list; (0,0) for empty tiles */
    const uint32_t* tile_order;  /* [tiles] dispatch order of the blend waves: a permutation, longest list classes first */
} SrBinningView;

typedef struct SrImageView {
    const float* final_T;       /* [3,H,W]: T_final, M1, M2 */
    const uint32_t* n_contrib;  /* [2,H,W]: last_contributor, median_contributor */
} SrImageView;

int sr_abi_version(void);
/* Which of the named compile-time switches (include/surfel_switches.h: SURVEY.md Appendix A's (!) items) this library was built with
 * at a NON-default value: SR_SWITCH_BITS, 0 for the shipped configuration. */
uint32_t sr_build_switches(void);
/* The content digest of the sources this library was built from (csrc/*, include/*.h, the build script; 16 hex digits, "unknown" for a build
 * that did not pass one): the in-tree build rebuilds on a mismatch and the Python loader refuses a library that is not its tree's. */
const char* sr_source_digest(void);
const char* sr_last_error(void);

/* Sizes of the three state buffers (bytes). num_rendered = D from sr_forward_plan. */
size_t sr_geom_bytes(int32_t P);
size_t sr_binning_bytes(int32_t P, uint32_t num_rendered, int32_t image_width, int32_t image_height);
size_t sr_image_bytes(int32_t image_width, int32_t image_height);
size_t sr_backward_workspace_bytes(int32_t P, uint32_t num_rendered, int32_t color_channels);

int sr_geom_view(void* geom, size_t geom_bytes, int32_t P, SrGeomView* out);
int sr_binning_view(void* binning, size_t binning_bytes, int32_t P, uint32_t num_rendered, int32_t image_width,
                    int32_t image_height, SrBinningView* out);
int sr_image_view(void* image, size_t image_bytes, int32_t image_width, int32_t image_height, SrImageView* out);

/* Forward, phase 1 (K1 preprocess + tile-count scan + depth ordering).
 * Writes radii[P] (int32) and the geometry state; returns D = number of (tile, Gaussian) duplicates in
 * *num_rendered_host after ONE host wait (the same read-back the reference does between its scan and duplicateWithKeys;
 * the depth sort is queued behind the copy of D, so the GPU keeps working while the caller sizes the binning buffer). */
int sr_forward_plan(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, int32_t* radii,
                    uint32_t* num_rendered_host, void* stream);

/* Forward, phase 2 (K3 / K4 expanding tile partition: column pass over the Gaussians, row pass over the column items; K5 ranges + dispatch
 * order; K6 blend).
 * out_color [NC,H,W], out_allmap [7,H,W] (0 sum w*depth, 1 alpha, 2-4 sum w*normal (view space),
 * 5 median depth, 6 distortion).
 * geom: the buffer sr_forward_plan of this frame filled.  It is required where there is anything to bin (P > 0 and num_rendered > 0), and
 * where the forward kernel is the one the device picks per frame, which reads the frame counts in it: the 16x16 tile with three colour
 * channels, no blend_counters and none of SR_FLAG_NO_QUADRANT_CULL, SR_FLAG_ROW_MAPPED_FORWARD, SR_FLAG_QUADRANT_MAPPED_FORWARD,
 * SR_FLAG_COOP_BACKWARD, SR_FLAG_ROW_BACKWARD (SR_FLAG_ONE_WAVE_BACKWARD and SR_FLAG_FORWARD_ONLY do not change the forward kernel).  NULL is
 * then refused (SR_ERR_INVALID_ARGUMENT, "geom is NULL") before anything is launched.  Otherwise it may be NULL; a buffer that is given is
 * held to sr_geom_bytes(P) like any other. */
int sr_forward_render(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning,
                      size_t binning_bytes, void* image, size_t image_bytes, uint32_t num_rendered,
                      float* out_color, float* out_allmap, void* stream);

/* Backward (K7 blend backward + K8 preprocess backward).  dL_dcolor [NC,H,W], dL_dallmap [7,H,W].
 * workspace: sr_backward_workspace_bytes(P, num_rendered, NC) bytes (one 96-B -- 112-B for NC = 9 -- gradient record + one flag byte per
 * (tile, Gaussian) duplicate), contents undefined on entry. */
int sr_backward(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                void* binning, size_t binning_bytes, void* image, size_t image_bytes, uint32_t num_rendered,
                const float* dL_dcolor, const float* dL_dallmap, void* workspace, size_t workspace_bytes,
                const SrGradients* grads, void* stream);

/* CONTRACT of every backward entry point (sr_backward, sr_backward_geometry, sr_class_backward): `frame` and the geometry inputs of `g`
 * (means3D, scales, rotations or transMat_precomp, activations, mask) must be BIT-IDENTICAL to those of the forward that filled the state
 * buffers.  K8 does not read Tu / Tv / Tw / the centre back from the 80-B record: it recomputes them from these inputs (the same device
 * functions as K1, hence the same bits) -- with other values the reference centre of K7's moment flush and K8's chain would silently
 * disagree.  The autograd shim saves and passes the forward's own tensors. */

/* The same backward in two halves, for callers that want to start a gradient exchange in between:
 *   sr_backward_blend     K7: per-(tile, Gaussian) gradient records into `workspace`;
 *   sr_backward_colors    optional, 3-channel pass: dL_dcolors[P,3] from those records alone (clamp-masked dL/drgb when shs is the
 *                         colour source = the input of sr_sh_gradient_expand; plain dL/dcolors_precomp otherwise) -- bit-identical
 *                         to what sr_backward_geometry returns in SrGradients.dL_dcolors;
 *   sr_backward_geometry  K8: everything else, from the same workspace.
 * sr_backward == sr_backward_blend + sr_backward_geometry. */
int sr_backward_blend(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                      void* image, size_t image_bytes, uint32_t num_rendered, const float* dL_dcolor, const float* dL_dallmap,
                      void* workspace, size_t workspace_bytes, void* stream);
int sr_backward_colors(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                       uint32_t num_rendered, void* workspace, size_t workspace_bytes, float* dL_dcolors, void* stream);
int sr_backward_geometry(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                         void* binning, size_t binning_bytes, void* image, size_t image_bytes, uint32_t num_rendered, void* workspace,
                         size_t workspace_bytes, const SrGradients* grads, void* stream);

/* Per-class distortion pass.  The reference's training iteration renders the same view once per semantic class
 * with the other classes boolean-indexed away and keeps only `rend_dist` of each (/root/reference/train.py:94-103 ->
 * gaussian_renderer/__init__.py:89-105, 165): five full rasterizations for five distortion maps.  This pass runs K1..K5 once and
 * returns all maps: out_dist[k] == allmap[6] of the operator called on the class-k subset (same list order, same thresholds, same
 * early termination per class), and the backward returns the gradients of all of them together.
 *   - class ids: colors_precomp[P,3], column 0 holds the class of a Gaussian as a float (0 .. n_classes-1; negative or >= n_classes =
 *     in no class, contributes nowhere); shs must be NULL.  sr_forward_plan is called first, exactly as for a render.
 *   - class_image: sr_class_image_bytes(W, H, n_classes) bytes of caller-owned state between forward and backward.
 *   - out_dist / dL_ddist: [n_classes, H, W].  grads: as sr_backward (dL_dcolors / dL_dsh are not produced: pass NULL).
 *   - every tile shape of the sweep; 1 <= n_classes <= 6. */
size_t sr_class_image_bytes(int32_t image_width, int32_t image_height, int32_t n_classes);
int sr_class_forward_render(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                            size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t num_rendered, float* out_dist,
                            void* stream);
int sr_class_backward(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* radii, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t num_rendered,
                      const float* dL_ddist, void* workspace, size_t workspace_bytes, const SrGradients* grads, void* stream);

/* The same per-class pass on the plan AND the binning of a colour pass of the same frame (SURVEY.md 8f N1 in full: K1..K5 once for the
 * colour render, the semantic channels and the per-class distortion maps; one K8 for all of their gradients):
 *   forward:  sr_forward_plan -> sr_forward_render (any colour configuration) -> sr_class_forward_shared
 *   backward: sr_backward_blend -> sr_class_backward_shared -> sr_backward_geometry
 * `classes` [P] int32 (negative or >= n_classes: in no class).  class_state: sr_class_shared_bytes(P, W, H, n_classes, num_rendered) bytes of
 * caller-owned state between forward and backward (per-class image state, class bytes, this pass's own hit masks; the class-ordered list
 * goes into a region of `binning` the colour pass no longer needs).  sr_class_backward_shared ADDS its gradient sums to the records
 * sr_backward_blend left in `workspace` (and starts records for duplicates only the class chains reached), so the one
 * sr_backward_geometry that follows returns the gradients of colour, allmap AND distortion maps together.  `g` / `frame` as given to
 * the colour pass (scales + rotations, no precomputed transMat). */
size_t sr_class_shared_bytes(int32_t P, int32_t image_width, int32_t image_height, int32_t n_classes, uint32_t num_rendered);
int sr_class_forward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* classes, void* geom, size_t geom_bytes,
                            void* binning, size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t num_rendered,
                            float* out_dist, void* stream);
int sr_class_backward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                             size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t num_rendered, const float* dL_ddist,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Frame-parallel SH gradient (no reference counterpart -- the reference is single-GPU).  The SH adjoint is
 * linear in the clamp-masked colour gradient and its only other per-view input is the camera position, so ranks that
 * rendered n_views frames of the SAME Gaussians all-gather dL_dcolors (12 B/Gaussian) instead of all-reducing dL_dsh
 * (192 B/Gaussian) and each expands the sum:  dL_dsh[i][k][c] = sum_v basis_k(dir(means3D[i], campos[v])) * dL_dcolors[v][i][c].
 * campos [n_views,3], dL_dcolors [n_views,P,3], dL_dsh [P,M,3] (fully written), all device pointers.  n_views = 1
 * reproduces sr_backward's dL_dsh bit for bit. */
int sr_sh_gradient_expand(int32_t P, int32_t sh_coeffs, int32_t sh_degree, int32_t n_views, const float* means3D,
                          const float* campos, const float* dL_dcolors, float* dL_dsh, void* stream);

/* K-nearest-neighbour mean squared distance == simple_knn._C.dist3knn / dist10knn (K = 3 / 10; scale
 * initialisation, /root/reference/scene/gaussian_model.py:16,151) and meanDistFromReferencePcd (distance of every point of
 * one cloud to another cloud, /root/reference/inpainting_pipeline/2_condition_preparation/2_generate_inpainted_mask.py:27,71-73).
 * out[i] = (sum of the K smallest squared distances from query i to the reference points) / K; with query == NULL every
 * reference point is searched against the OTHER reference points (n_query ignored, out [n_reference]).  Exact search.
 * points are [n,3] float32 device arrays; workspace: sr_knn_workspace_bytes(n_query or 0, n_reference) bytes. */
size_t sr_knn_workspace_bytes(int32_t n_query, int32_t n_reference);
int sr_knn_mean_dist2(int32_t n_query, const float* query, int32_t n_reference, const float* reference, int32_t K,
                      int32_t take_sqrt, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Radius clustering == GaussianModel.cluster_instance_with_mask / cluster_semantic_instance with parallel=False
 * (/root/reference/scene/gaussian_model.py:579-651): the connected components of the graph that joins two active points when
 * sqrtf((dx*dx + dy*dy) + dz*dz) < radius in float32 (strictly below), each named by its smallest point index.
 * labels[i] = that index for an active point, -1 for a point with active[i] == 0, i for an active point with a NaN / inf coordinate
 * (it is within range of nobody, itself included).  xyz [n,3] float32, active [n] uint8 or NULL (every point), labels [n] int64: device
 * arrays; workspace: sr_cluster_workspace_bytes(n) bytes.  Exact and deterministic; a cloud whose points all lie within one radius of
 * each other costs all its pairs.  SR_ERR_INVALID_ARGUMENT for n < 0, a radius that is not a finite number >= 0, or NULL xyz / labels /
 * workspace with n > 0; SR_ERR_BUFFER_TOO_SMALL for a short workspace.
 * Added without a new SR_ABI_VERSION: nothing that existed changed its signature, layout or meaning, so a caller built against the
 * header before these two declarations runs unchanged against this library (a caller that needs them checks for the symbols). */
size_t sr_cluster_workspace_bytes(int32_t n);
int sr_cluster_radius(int32_t n, const float* xyz, const uint8_t* active, float radius, int64_t* labels, void* workspace,
                      size_t workspace_bytes, void* stream);

/* K9: present[i] = (view-space z of means3D[i] > 0.2).  present is uint8 (torch.bool storage). */
int sr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, void* stream);

/* Fused post-processing of the operator's allmap == gaussian_renderer/__init__.py:152-177 +
 * utils/point_utils.py:9-37 of the reference: allmap[7,H,W] -> rend_normal[3,H,W] (world space), surf_depth[1,H,W],
 * surf_normal[3,H,W] (finite-difference pseudo-normals times alpha, zero border), surf_point[3,H,W].
 * fovx/fovy in radians, viewmatrix = world_view_transform (device [16]).  Backward: gradient w.r.t. allmap from the
 * gradients of the four outputs (NULL = zero); scratch6 is [6,H,W] floats of caller-owned scratch; channel 6 of
 * g_allmap is written as 0 and alpha is treated as detached inside surf_normal, as in the reference. */
int sr_postprocess_forward(int32_t image_width, int32_t image_height, float fovx, float fovy, float depth_ratio,
                           const float* viewmatrix, const float* allmap, float* rend_normal, float* surf_depth,
                           float* surf_normal, float* surf_point, void* stream);
int sr_postprocess_backward(int32_t image_width, int32_t image_height, float fovx, float fovy, float depth_ratio,
                            const float* viewmatrix, const float* allmap, const float* g_rend_normal, const float* g_surf_depth,
                            const float* g_surf_normal, const float* g_surf_point, float* scratch6, float* g_allmap, void* stream);

/* Fused photometric loss of a training iteration == train.py:113-119 + utils/loss_utils.py:18-64 of the reference:
 *     x = image (+ sky * (1 - alpha));  l1 = mean|x - gt|;  ssim = mean of the SSIM map of (x, gt);
 *     loss = (1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim)
 * SSIM with the reference's 11-tap Gaussian window (sigma 1.5), zero padding of 5 pixels (not renormalised at the border),
 * C1 = 0.01^2, C2 = 0.03^2.  image, gt, sky are [C,H,W], alpha is [1,H,W]; sky and alpha may be NULL together (no composite).
 * Forward: writes out3 = {loss, l1, ssim} on the device (no read-back, no float atomics: two calls give the same bits) and keeps
 * three [C,H,W] planes of SSIM derivatives in the workspace (sr_image_loss_workspace_bytes(W, H, C) bytes, caller-owned).
 * Backward: from the same inputs, the workspace the forward filled and the upstream scalar g_loss (a DEVICE float), writes
 * g_image[C,H,W] and, with the composite, g_sky[C,H,W] and g_alpha[1,H,W] (alpha is not detached, as in the reference); gt gets
 * no gradient.  Bad sizes, a missing pointer, only one of sky / alpha or a short workspace are refused before any launch. */
size_t sr_image_loss_workspace_bytes(int32_t image_width, int32_t image_height, int32_t channels);
int sr_image_loss_forward(int32_t image_width, int32_t image_height, int32_t channels, float lambda_dssim, const float* image,
                          const float* gt, const float* sky, const float* alpha, void* workspace, size_t workspace_bytes,
                          float* out3, void* stream);
int sr_image_loss_backward(int32_t image_width, int32_t image_height, int32_t channels, float lambda_dssim, const float* image,
                           const float* gt, const float* sky, const float* alpha, const void* workspace, size_t workspace_bytes,
                           const float* g_loss, float* g_image, float* g_sky, float* g_alpha, void* stream);

/* The other losses of a training iteration == train.py:87-88 and :124-143 of the reference (and 1_optimization.py:249-256 of its
 * unveiling stage), csrc/aux_loss.hip.  Every forward is one kernel of per-workgroup partial sums + one workgroup that adds them in a
 * fixed order; every backward is one kernel that reads the upstream scalar g_loss from DEVICE memory.  The arithmetic is float64 on
 * float32 data: each loss and each gradient element is the float64 value of its expression rounded to float32 once.  No atomics (two
 * calls give the same bits), no host read-back, nothing allocated: the caller owns the workspace of sr_aux_loss_workspace_bytes(n)
 * bytes, n = the pixels (W * H) or Gaussians (P) of the call; only the forwards use it, and nothing in it is kept for the backward.
 *
 * sr_semantic_ce_*: logits x [C,H,W], C <= SR_CE_MAX_CLASSES; weight = C HOST floats read during the call (NULL: all ones) and carried
 * in the launch, so a captured graph replays them.  label_bytes selects the target: 0 = probabilities t [C,H,W] float32, term
 * -sum_c w_c t_c (x_c - lse(x)); 1 / 4 / 8 = an [H,W] label map of uint8 / int32 / int64, term -w[l] (x[l] - lse(x)), where a label
 * outside 0..C-1 gives 0 * lse(x) (the all-zero one-hot row of the reference).  out1[0] = (sum of terms) / (W * H) ==
 * F.cross_entropy(x[None], t[None], weight=w): with probability targets torch divides by the pixel count, not by the weights' sum.
 * g_logits[c] = (g / N) (softmax_c S - w_c t_c), S = sum_k w_k t_k (labels: w[l], or 0 outside the range).
 * Differences from torch, on purpose: with LABELS an -inf logit of another class leaves the term finite (torch's one-hot product forms
 * 0 * -inf = NaN; the probability form does that too); a NaN logit of any class makes the loss NaN in both forms.
 *
 * sr_surface_reg_*: rend_normal, surf_normal [3,H,W], rend_dist [1,H,W]; normal = mean(1 - sum_c rn_c sn_c), dist = mean(rend_dist);
 * out3 = {lambda_normal normal + lambda_dist dist, lambda_normal normal, lambda_dist dist}.  The backward writes the gradients whose
 * pointers are given: g_rend_normal = -(g lambda_normal / N) surf_normal, g_surf_normal = -(g lambda_normal / N) rend_normal,
 * g_rend_dist = g lambda_dist / N; the two normal maps are needed only where one of their gradients is asked for, rend_dist never.  A
 * weight of 0 is not special: the maps are read and multiplied by it.
 *
 * sr_opacity_shrink_*: out1[0] = mean(sigmoid(opacity[P])) of RAW opacities, g = (g / P) s (1 - s); activated != 0: the values are
 * opacities already, mean(opacity) and g / P.
 *
 * SR_ERR_INVALID_ARGUMENT before any launch for W, H or P < 1, C outside 1..SR_CE_MAX_CLASSES, a label_bytes other than 0, 1, 4, 8 and
 * a missing pointer; SR_ERR_BUFFER_TOO_SMALL for a short workspace; SR_ERR_UNSUPPORTED for more than 2^31 - 1 workgroups of 256
 * elements.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
#define SR_CE_MAX_CLASSES 8
size_t sr_aux_loss_workspace_bytes(int64_t n);
int sr_semantic_ce_forward(int32_t image_width, int32_t image_height, int32_t classes, const float* logits, const void* target,
                           int32_t label_bytes, const float* weight, void* workspace, size_t workspace_bytes, float* out1, void* stream);
int sr_semantic_ce_backward(int32_t image_width, int32_t image_height, int32_t classes, const float* logits, const void* target,
                            int32_t label_bytes, const float* weight, const float* g_loss, float* g_logits, void* stream);
int sr_surface_reg_forward(int32_t image_width, int32_t image_height, const float* rend_normal, const float* surf_normal,
                           const float* rend_dist, double lambda_normal, double lambda_dist, void* workspace, size_t workspace_bytes,
                           float* out3, void* stream);
int sr_surface_reg_backward(int32_t image_width, int32_t image_height, const float* rend_normal, const float* surf_normal,
                            double lambda_normal, double lambda_dist, const float* g_loss, float* g_rend_normal, float* g_surf_normal,
                            float* g_rend_dist, void* stream);
int sr_opacity_shrink_forward(int64_t P, const float* opacity, int32_t activated, void* workspace, size_t workspace_bytes, float* out1,
                              void* stream);
int sr_opacity_shrink_backward(int64_t P, const float* opacity, int32_t activated, const float* g_loss, float* g_opacity, void* stream);

/* The per-pixel part of the sky model == SkyModel.render_with_camera of the reference's scene/env_map.py with its constructor defaults,
 * csrc/sky.hip.  Every pixel of a frame hands that model the same position, so the caller folds the 95 position channels of the first
 * layer into one vector c[64] = W0[:, 16:] feat + b0 and these calls do what differs per pixel, in float32:
 *   dir = R ((i - cx) / fx, -(j - cy) / fy, -1) for pixel column i, row j (NOT normalised);  sh[16] = torch-ngp's degree-4 shencoder of dir;
 *   out[:, j, i] = sigmoid(W3 relu(W2 relu(W1 relu(W0sh sh + c) + b1) + b2) + b3).
 * cam: 13 device floats {fx, fy, cx, cy, R[9] row-major (c2w[:3, :3])}; w0sh [64,16] (the SH columns of the first layer), c [64],
 * w1, w2 [64,64], b1, b2 [64], w3 [3,64], b3 [3], all row-major device float32; out and g_out [3,H,W].
 * sr_sky_forward keeps nothing for the backward.  sr_sky_backward recomputes the activations and writes the gradients whose pointers
 * are given (NULL: not wanted; none wanted: no work), shaped like their weights; cam gets no gradient.  No atomics: a grid of at most
 * max_workgroups workgroups (0: the library's default) sweeps the image 256 pixels at a time, each workgroup keeps ONE float64 set of
 * the 9603 sums, stores it to the workspace, and a second kernel adds the sets in index order and rounds once.  The workspace,
 * sr_sky_workspace_bytes(max_workgroups) bytes, therefore depends on the workgroup count and not on W * H; two calls with equal
 * arguments give equal bits, another max_workgroups another order of the same sum.  relu keeps a NaN; its derivative passes the
 * gradient unless the activation is <= 0, as torch's does.
 * SR_ERR_INVALID_ARGUMENT before any launch for W or H < 0, max_workgroups outside 0..65536, a NULL cam or weight, a NULL out / g_out
 * or workspace with work to do; SR_ERR_BUFFER_TOO_SMALL for a short workspace; SR_ERR_UNSUPPORTED for 2^31 pixels or more.  W * H == 0
 * is no error and no work.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_sky_workspace_bytes(int32_t max_workgroups);
int sr_sky_forward(int32_t image_width, int32_t image_height, const float* cam, const float* w0sh, const float* c, const float* w1,
                   const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, int32_t max_workgroups, float* out,
                   void* stream);
int sr_sky_backward(int32_t image_width, int32_t image_height, const float* cam, const float* w0sh, const float* c, const float* w1,
                    const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const float* g_out,
                    int32_t max_workgroups, void* workspace, size_t workspace_bytes, float* g_w0sh, float* g_c, float* g_w1, float* g_b1,
                    float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* stream);

/* One Adam step over up to SR_ADAM_MAX_SEGMENTS float32 tensors in ONE launch == torch.optim.Adam (no weight decay, no amsgrad, not
 * maximising) as the reference builds it in scene/gaussian_model.py:171-180 and steps it in train.py:197.  Per element, in float32 and
 * in the order of torch's single-tensor path, with correctly rounded division and square root and no contraction:
 *     m = m + (g - m) * (1 - beta1);   v = v * beta2 + ((1 - beta2) * g) * g;
 *     denom = sqrt(v) / bc2_sqrt + eps;   p = p - step_size * (m / denom)
 * The caller forms step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) per tensor in double (t = that tensor's step count,
 * this step included) and stores them rounded to float32.  beta1, beta2 and eps arrive as DOUBLES and are rounded once inside, together
 * with the complements 1 - beta formed in double: float(1 - float(0.999)) is 1.3e-5 away from float(0.001), which a float32 beta would
 * make the weight of g*g.  Each tensor is n contiguous floats behind param / grad / exp_avg / exp_avg_sq (4-B aligned; a tensor whose
 * four pointers are 16-B aligned moves 16 B per lane and access); n = 0 is allowed and skipped.  The work is cut into chunks of
 * SR_ADAM_CHUNK elements.  No atomics: two calls on equal inputs give equal bits; a NaN / Inf gradient element touches its element only.
 * The hyper-parameters travel by value in the launch: a captured graph would replay THIS step's step_size. */
#define SR_ADAM_MAX_SEGMENTS 8
#define SR_ADAM_CHUNK 4096
typedef struct SrAdamSegment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    float step_size;
    float bc2_sqrt;
} SrAdamSegment;
int sr_adam_step(const SrAdamSegment* segments, int32_t n_segments, double beta1, double beta2, double eps, void* stream);

/* sr_adam_step restricted to the rows a mask selects: the optimizer step of the masked re-optimisation model (the reference's
 * MaskGaussianModel, scene/mask_gaussian.py:195-209), whose six trainable deltas move only around the removed object.  Each tensor is
 * n = P * row_len contiguous floats (row_len >= 1, below 2^30); mask is uint8 [P] (torch.bool storage), one for all tensors of the call.
 * An element whose row has mask == 0 is neither read nor written -- not param, grad, exp_avg or exp_avg_sq: a 16-B group that straddles
 * a selected and an unselected row leaves the unselected elements bit for bit as they were, and what an unselected row of grad holds
 * (NaN included) is never seen.  Every other element goes through the very update of sr_adam_step (one function in csrc/optimizer.hip).
 * CONTRACT: this equals the dense step wherever the skipped rows have zero gradient and zero moments and eps > 0 -- Adam then leaves
 * such a row's parameter, exp_avg and exp_avg_sq exactly as they are (m = 0, v = 0, p - step_size * (0 / eps) = p).  In the reference
 * that is every masked-out row: set_mask precedes training_setup, which creates the moments as zeros; a masked-out row's gradient is
 * delta-gradient * 0; and reset_mask builds a new optimizer.  A caller that changes the mask under a live optimizer state freezes the
 * moments of the rows it switches off instead of letting them decay.
 * SR_ERR_INVALID_ARGUMENT for P < 0, a NULL mask with P > 0, a row_len outside [1, 2^30), n != P * row_len and everything sr_adam_step
 * refuses; P == 0 (every n == 0) is no error and no work.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
typedef struct SrAdamRowSegment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    float step_size;
    float bc2_sqrt;
    int64_t row_len;
} SrAdamRowSegment;
int sr_adam_step_rows(const SrAdamRowSegment* segments, int32_t n_segments, int32_t P, const uint8_t* mask, double beta1, double beta2,
                      double eps, void* stream);

/* The getters of the masked re-optimisation model == MaskGaussianModel.get_xyz / get_features / get_opacity / get_scaling / get_rotation
 * of the reference (scene/mask_gaussian.py:139-176) BEFORE their activations, for all six properties in one launch, and their adjoint in
 * one more (csrc/mask_model.hip).  base and delta are the six tensors of P Gaussians with M = sh_coeffs SH coefficients: xyz [P,3],
 * features_dc [P,1,3], features_rest [P,M-1,3] (zero-sized and never read for M == 1), opacity [P,1], scaling [P,2], rotation [P,4];
 * mask is uint8 [P]; fixed_bits has the reference's MASK_PROPERTY bit order (SR_MASK_FIXED_*).
 * sr_mask_compose writes the effective raw tensors xyz [P,3], features [P,M,3] (the concatenation of the two SH parts), opacity, scaling,
 * rotation:  a row with mask != 0 gets base + delta; a row with mask == 0 gets base + 0.0f and its delta row is NOT read; a fixed property
 * gets its base bit for bit and its delta pointer is not read (each half of features on its own).  An output pointer may be NULL where
 * its property is fixed (features: where both halves are): the caller then uses the base tensor itself.
 * Two deliberate differences from the reference's `base + delta * mask`: a non-finite delta in a masked-out row does not reach the output
 * (the reference yields NaN there), and a zero may differ in sign (-0.0f + 0.0f is +0.0f; the reference adds delta * 0, which is -0.0f
 * for a negative delta).
 * sr_mask_compose_backward writes the gradients of the deltas from the upstream gradients of the five outputs: a row with mask != 0 gets
 * the upstream row (features split back into dc and rest), a row with mask == 0 gets zeros and its upstream row is NOT read.  A d_delta
 * pointer may be NULL (not wanted); one that is given needs its upstream gradient and a property that is not fixed.  base gets no
 * gradient here (the model freezes it; it would be the upstream gradient itself).
 * float32, contiguous, 4-B aligned (16-B aligned tensors move 16 B per lane where their rows allow it); no LDS, no atomics, no workspace:
 * equal inputs give equal bits.  Both check every argument before their first HIP call: SR_ERR_INVALID_ARGUMENT for P < 0,
 * sh_coeffs < 1, fixed_bits above 63, a missing struct, mask or tensor; SR_ERR_UNSUPPORTED for P * 3 * sh_coeffs >= 2^31.  P == 0 is no
 * error and no work.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
#define SR_MASK_FIXED_XYZ 1
#define SR_MASK_FIXED_FEATURES_DC 2
#define SR_MASK_FIXED_FEATURES_REST 4
#define SR_MASK_FIXED_SCALING 8
#define SR_MASK_FIXED_ROTATION 16
#define SR_MASK_FIXED_OPACITY 32
typedef struct SrMaskTensors {    /* the six per-Gaussian tensors, in the order of the reference's training_setup */
    float* xyz;
    float* features_dc;
    float* features_rest;
    float* opacity;
    float* scaling;
    float* rotation;
} SrMaskTensors;
typedef struct SrMaskEffective {  /* the five tensors the renderer reads */
    float* xyz;
    float* features;
    float* opacity;
    float* scaling;
    float* rotation;
} SrMaskEffective;
int sr_mask_compose(int32_t P, int32_t sh_coeffs, const SrMaskTensors* base, const SrMaskTensors* delta, const uint8_t* mask,
                    uint32_t fixed_bits, const SrMaskEffective* out, void* stream);
int sr_mask_compose_backward(int32_t P, int32_t sh_coeffs, const SrMaskEffective* upstream, const uint8_t* mask, uint32_t fixed_bits,
                             const SrMaskTensors* d_delta, void* stream);

/* Densification statistics of one rendered view == train.py:168-169 + scene/gaussian_model.py:555-557 of the reference, with
 * visibility_filter = radii > 0.  For every i < P with radii[i] > 0:
 *     xyz_gradient_accum[i] += sqrt(gx^2 + gy^2 + gz^2) of viewspace_grad[i] ([P,3]);   denom[i] += 1;
 *     max_radii2D[i] = max(max_radii2D[i], (float)radii[i])
 * Rows with radii <= 0 are neither read nor written.  One kernel, no temporaries, no host synchronisation. */
int sr_densification_stats(int32_t P, const float* viewspace_grad, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                           float* max_radii2D, void* stream);

/* Densify-and-prune of the Gaussians and their Adam moments == GaussianModel.densify_and_prune with densify_and_clone, densify_and_split,
 * densification_postfix, cat_tensors_to_optimizer, _prune_optimizer and prune_points of the reference (scene/gaussian_model.py:402-553),
 * as one decision pass, one scan and one gather: every surviving row moves once.  Two calls with one host read-back between them.
 *
 * sr_densify_plan decides, per Gaussian i < P, in float32 (correctly rounded division; exp / log / sigmoid of the device library):
 *     grad   = accum[i] / denom[i], NaN -> 0 (0/0 gives 0; x/0 with x > 0 stays +inf)
 *     big    = max(exp(scaling[i][0]), exp(scaling[i][1]))                      (scaling is the raw [P,2] parameter)
 *     clone  = |grad| >= max_grad && big <= percent_dense_extent;   split = grad >= max_grad && big > percent_dense_extent
 *              (the reference tests the norm for the clone and the signed value for the split; accum is a sum of norms in training)
 *     pruned = sigmoid(opacity[i]) < min_opacity || (prune_mask && prune_mask[i]) || (ws_limit >= 0 && big > ws_limit)
 * a clone shares its parent's fate; the two children of a split parent share one, with their own scale exp(log(exp(s) / 1.6)) in the
 * world-size test.  max_grad = +inf (or NaN) selects nothing, and only then may accum and denom be NULL: with min_opacity = -inf and
 * ws_limit < 0 the pair of calls is a plain prune_points(prune_mask).  The reference's `max_radii2D > max_screen_size` test is not
 * here because it never holds there: densification_postfix zeroes max_radii2D before the prune reads it; a max_screen_size only
 * switches the world-size test on (ws_limit = 0.1 * extent, else negative).
 * It leaves in the workspace (sr_densify_workspace_bytes(P) bytes, device memory, 256-B aligned):
 *     offset 0                          uint8  flags[P]        SR_DENSIFY_FLAG_* bits
 *     offset align256(P)                uint32 source_map[2P]  per OUTPUT row: source index | kind << 30 (SR_DENSIFY_KIND_*)
 *     offset align256(P) + align256(8P) uint32 child_rank[P]   per kept child pair: its parent's rank among the split-selected
 * and returns counts_out[4] = {kept originals K, kept clones C, split-selected S, kept child pairs H} (host memory; the call waits for
 * the stream once).  Output order: the K surviving originals that were not split in index order, the C surviving clones, the H
 * surviving first children, the H surviving second children: P_out = K + C + 2 H rows.  Exclusive scans, no atomics: deterministic.
 *
 * sr_densify_apply gathers up to SR_DENSIFY_MAX_SEGMENTS tensors of row_words 32-bit words per row from src [P rows] to dst [P_out rows]
 * in one launch, each tensor walked as a flat stream of output words.  Roles:
 *     COPY     every row is its source row, bit for bit (parameters of clones and children, int32 rows)
 *     MOMENT   an original's row is copied, a new row (clone, child) is zeros
 *     XYZ      row_words == 3; a child's row is R(rotation / |rotation|) (exp(s0) n0, exp(s1) n1, 0) + xyz with (n0, n1) = noise row
 *              k * S + j of noise[2S,2] for child k of the j-th split-selected Gaussian; rotation [P,4], scaling [P,2]: the SOURCE arrays
 *     SCALING  row_words == 2; a child's value is log(exp(s) / 1.6)
 * row_words == 0 is legal and moves nothing; row_words <= 65535.  counts are the four words sr_densify_plan returned for this workspace.
 * Both calls check every argument before their first HIP call, run on the caller's stream and allocate nothing; P == 0 is no error and
 * no work; P < 2^30.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
#define SR_DENSIFY_MAX_SEGMENTS 8
#define SR_DENSIFY_FLAG_CLONE 1
#define SR_DENSIFY_FLAG_SPLIT 2
#define SR_DENSIFY_FLAG_KEEP_SELF 4   /* the row itself survives (never set on a split parent); its clone, if any, survives with it */
#define SR_DENSIFY_FLAG_KEEP_CHILD 8  /* split, and both children survive */
#define SR_DENSIFY_KIND_ORIGINAL 0
#define SR_DENSIFY_KIND_CLONE 1
#define SR_DENSIFY_KIND_CHILD0 2
#define SR_DENSIFY_KIND_CHILD1 3
#define SR_DENSIFY_ROLE_COPY 0
#define SR_DENSIFY_ROLE_MOMENT 1
#define SR_DENSIFY_ROLE_XYZ 2
#define SR_DENSIFY_ROLE_SCALING 3
typedef struct SrDensifySegment {
    const void* src;     /* [P, row_words] 32-bit words */
    void* dst;           /* [P_out, row_words] */
    int32_t row_words;
    int32_t role;        /* SR_DENSIFY_ROLE_* */
} SrDensifySegment;
size_t sr_densify_workspace_bytes(int32_t P);
int sr_densify_plan(int32_t P, const float* accum, const float* denom, const float* opacity, const float* scaling, float max_grad,
                    float min_opacity, float percent_dense_extent, float ws_limit, const uint8_t* prune_mask, void* workspace,
                    size_t workspace_bytes, uint32_t* counts_out, void* stream);
int sr_densify_apply(int32_t P, const uint32_t* counts, const float* noise, const float* rotation, const float* scaling,
                     const SrDensifySegment* segments, int32_t n_segments, void* workspace, size_t workspace_bytes, void* stream);

/* TSDF fusion of rendered depth maps on a list of samples or on a regular grid (csrc/tsdf.hip): what the reference's unbounded mesh
 * export evaluates on its marching-cubes samples (utils/mesh_utils.py:181-234, compute_sdf_perframe + compute_unbounded_tsdf), one thread
 * per sample with the loop over the V views inside the kernel.
 * Per sample tsdf = 1, weight = 1, rgb = 0 to begin with (the reference's start values: its running average begins with a phantom
 * observation of +1); then per view v in view order:
 *     q = [x y z 1] full_proj[v] (row vector times matrix), zc = q.w, pix = q.xy / zc;
 *     the view is skipped unless -1 < pix.x < 1, -1 < pix.y < 1 and zc > 0 (strict; a NaN is false);
 *     depth (and colour) = grid_sample(bilinear, align_corners = True) at pix: ix = (pix.x + 1) / 2 * (W - 1), the four taps summed in the
 *     order nw, ne, sw, se; an in-bounds tap is multiplied in even with weight 0, a tap with an index out of bounds is not read;
 *     sdf = depth - zc; the view is skipped unless sdf > -trunc (a NaN is false); else, with s = clamp(sdf / trunc, -1, 1):
 *     tsdf = (tsdf w + s) / (w + 1), rgb = (rgb w + colour) / (w + 1), w += 1.
 * trunc = (float)(5 voxel_size).  With space.contract the sample y is in contracted space: its world point is
 * uncontract(y) radius + center, uncontract(y) = y for |y| < 1, else 1 / (2 - |y|) * (y / |y|); that point is what is projected, and
 * trunc is multiplied by 1 / (2 - min(|world point|, 1.9)) where |world point| > 1 -- the norm of the un-normalised world point, as the
 * reference's line 201 takes it.
 * views.channels == 1: maps is [V,H,W] depths and rgb must be NULL; views.channels == 4: maps is [V,H,W,4] records (depth, r, g, b),
 * 16-B aligned, one load per tap.  Outputs: tsdf [n], rgb [n,3] or NULL, weight [n] or NULL (weight - 1 = the views that integrated the
 * sample).  All offsets into maps are 64-bit.
 * sr_tsdf_fuse reads n samples [n,3].  sr_tsdf_fuse_grid generates them: sample (ix, iy, iz) of a dims[0] x dims[1] x dims[2] grid is
 * fmaf(i, step[axis], lo[axis]) per axis, for ix in [ix_begin, ix_end); the outputs hold (ix_end - ix_begin) dims[1] dims[2] samples,
 * sample (ix, iy, iz) at ((ix - ix_begin) dims[1] + iy) dims[2] + iz: the flattening of torch.meshgrid(indexing="ij").
 * Both check every argument before their first HIP call (SR_ERR_INVALID_ARGUMENT: a NULL pointer, V < 1, H or W < 2, voxel_size <= 0 or
 * NaN, a slab outside the grid; SR_ERR_UNSUPPORTED: 2^31 samples or more in one call), run on the caller's stream, allocate nothing and
 * read nothing back; no atomics: equal inputs give equal bits.  n == 0 (an empty slab) is no error and no work.
 * Added without a new SR_ABI_VERSION: nothing that existed changed. */
typedef struct SrTsdfViews {
    const float* maps;        /* device [V,H,W] (channels 1) or [V,H,W,4] (channels 4) */
    const float* full_proj;   /* device [V,16]: full_proj_transform of every view, row-major as the reference stores it */
    int32_t V, H, W, channels;
} SrTsdfViews;
typedef struct SrTsdfSpace {
    double voxel_size;
    int32_t contract;         /* 0: world-space samples, constant truncation (center and radius are not read) */
    float center[3];
    float radius;
} SrTsdfSpace;
int sr_tsdf_fuse(const SrTsdfViews* views, const SrTsdfSpace* space, int32_t n, const float* samples, float* tsdf, float* rgb, float* weight,
                 void* stream);
int sr_tsdf_fuse_grid(const SrTsdfViews* views, const SrTsdfSpace* space, const int32_t* dims, const float* lo, const float* step,
                      int32_t ix_begin, int32_t ix_end, float* tsdf, float* rgb, float* weight, void* stream);

/* Marching cubes on a resident float32 volume (csrc/mesh.hip; the case table and its conventions: csrc/mc_table.h, derived by
 * tools/make_mc_table.py): volume [dims[0], dims[1], dims[2]] with the last axis fastest -- what sr_tsdf_fuse_grid fills -- -> an indexed,
 * welded triangle mesh, vertices [Nv,3] float32 and faces [Nf,3] int32.  Two calls with one host read-back between them, which is the
 * caller's: sr_mesh_count leaves counts[2] = {Nv, Nf} in DEVICE memory; the caller reads them, allocates and calls sr_mesh_emit with the
 * same volume, dims, level and workspace (sr_mesh_workspace_bytes(dims) bytes of device memory, 16-B aligned: 5 bytes a grid point + 16
 * per 4096 grid points; 0 for dims no call accepts).
 *     inside means value < level, strictly; grid point (ix, iy, iz) has the linear index (ix dims[1] + iy) dims[2] + iz;
 *     a grid point OWNS the vertex of each of its three forward edges (axis x, y, z) whose two ends are finite and differ in `inside`;
 *     the cell whose lowest corner a grid point is yields the triangles of its case (bit c = corner c inside) iff its eight corners are
 *     finite; an edge with a NaN or inf end owns no vertex, a cell with such a corner emits no triangle;
 *     vertices ascend by (linear index of the owning point, axis x < y < z), faces by (linear index of the cell's lowest corner, order
 *     in the table); a face holds vertex indices; its normal (right-hand rule) points towards the larger values;
 *     the vertex on the edge from grid point i to i + 1 along an axis: t = (level - a) / (b - a) in float32 (IEEE division), a the value
 *     at i; its coordinate along that axis is fmaf(i + t, step[axis], lo[axis]), the other two are fmaf(index, step, lo) -- the grid
 *     points of sr_tsdf_fuse_grid.  A vertex at t == 0 or t == 1 is kept: zero-area triangles are legal, the topology stays closed.
 *     With space != NULL and space->contract != 0 each vertex y is then replaced by uncontract(y) radius + center as sr_tsdf_fuse states
 *     it (voxel_size is not read); else the vertices stay in grid coordinates.
 * A grid with an axis of length 1 has no cells: an empty mesh (counts = {0, 0}), no error.  Exclusive prefix sums, no atomics: equal
 * inputs give equal bits.  A count reads 0xFFFFFFFF where Nv or 3 Nf does not fit in int32: no mesh this ABI can index.
 * Both calls check every argument before their first HIP call (SR_ERR_INVALID_ARGUMENT: a NULL pointer, a non-positive dim, a NaN level,
 * a workspace too small or not 16-B aligned, a negative count, faces without vertices; SR_ERR_UNSUPPORTED: 2^31 grid points or more,
 * 3 n_faces beyond int32), run on the caller's stream, allocate nothing and read nothing back.  All offsets into the volume are 64-bit.
 * Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_mesh_workspace_bytes(const int32_t* dims);
int sr_mesh_count(const float* volume, const int32_t* dims, float level, void* workspace, size_t workspace_bytes, uint32_t* counts,
                  void* stream);
int sr_mesh_emit(const float* volume, const int32_t* dims, float level, const float* lo, const float* step, const SrTsdfSpace* space,
                 void* workspace, size_t workspace_bytes, int32_t n_vertices, int32_t n_faces, float* vertices, int32_t* faces, void* stream);

/* Mesh post-processing (csrc/mesh_post.hip): what the reference's post_process_mesh does with every mesh it writes
 * (utils/mesh_utils.py:23-44, through open3d: cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices,
 * remove_degenerate_triangles) on an indexed mesh resident on the GPU: faces [nf,3] int32 over nv vertices [nv,3] float32, with optional
 * colours [nv,3] float32.  All pointers are device pointers; workspace: sr_mesh_post_workspace_bytes(nv, nf) bytes, 16-B aligned (28 bytes a
 * face + 4 a vertex; 0 for counts no call accepts).
 *   Edges and components.  An edge of face (a, b, c) is the unordered index pair of (a, b), (b, c) or (c, a) -- a pair of equal indices is
 *     an edge like any other.  Two faces are adjacent when they have an equal edge: in either winding, for any number of faces on one edge
 *     and for duplicate faces; sharing only a vertex joins nothing.  A component is named by its smallest face index: labels[f];
 *     sizes[r] = the face count of the component at its root r, 0 at every other face.  The dense cluster id of a component is the rank
 *     of its root among the roots -- the order in which a sweep over the faces from 0 upwards meets the components.  That should also be
 *     open3d's numbering; this has not been verified against open3d.
 *   Threshold (the caller's: a device word, so that no host synchronisation is needed for it).  With n = the k-th largest value of sizes
 *     over all nf entries, zeros included, k = min(cluster_to_keep, nf): threshold = max(n, min_triangles), min_triangles = 50 in the
 *     reference.  A face goes when its component's size is < threshold, strictly, so ties at the k-th place all stay.  With fewer
 *     components than cluster_to_keep, n is 0 and the floor decides: every component of at least min_triangles faces stays (the
 *     reference's np.sort(...)[-cluster_to_keep] raises IndexError there: a deliberate difference).
 *   Order of the removals, as open3d runs them: (1) the faces of the small components; (2) the vertices no remaining face references,
 *     their colours with them; (3) the faces with two equal indices.  A vertex that only a degenerate face of a kept component references
 *     therefore stays.  Surviving vertices and faces keep their relative order; vertex and colour rows are copied word for word; the only
 *     atomics are integer additions and the union-find's compare-and-swap under the smaller root: equal inputs give equal bits.
 *   A face with an index outside [0, nv) is never used to address memory: it is counted, is a component of its own and is never kept.
 *   cluster_area, open3d's third result, is not computed (the reference does not read it).
 * sr_mesh_components: labels [nf], sizes [nf], n_out_of_range [1].  sr_mesh_filter_count: from labels and sizes (in [0, nf) or the face is
 * not kept) and *threshold, counts[3] = {nv_out, nf_out, n_out_of_range} in DEVICE memory -- the one read-back, which is the caller's;
 * sr_mesh_filter_emit, with the same faces, nv, nf and workspace and the two counts read: vertices_out [nv_out,3], colors_out [nv_out,3]
 * where colors is not NULL, faces_out [nf_out,3] renumbered.
 * Cost: a half-edge walks the bucket of its lower vertex, so a vertex of valence d costs about 2 d^2 reads: small on a marching-cubes
 * mesh (d about 6), slow and still right at a hub vertex.
 * nf == 0 or nv == 0 is no error and no work: counts = {0, 0, 0}, nothing is emitted (sr_mesh_components writes nothing for nf == 0 and
 * refuses nf > 0 with nv == 0, where no face has a label to give).  All three check every argument before their first HIP call
 * (SR_ERR_INVALID_ARGUMENT: a negative count, a NULL or misaligned pointer, nv_out > nv, nf_out > nf, faces without vertices;
 * SR_ERR_BUFFER_TOO_SMALL: a short workspace; SR_ERR_UNSUPPORTED: 3 nf beyond int32), run on the caller's stream and allocate nothing.
 * Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_mesh_post_workspace_bytes(int32_t nv, int32_t nf);
int sr_mesh_components(const int32_t* faces, int32_t nv, int32_t nf, int32_t* labels, int32_t* sizes, uint32_t* n_out_of_range, void* workspace,
                       size_t workspace_bytes, void* stream);
int sr_mesh_filter_count(const int32_t* faces, int32_t nv, int32_t nf, const int32_t* labels, const int32_t* sizes, const int32_t* threshold,
                         void* workspace, size_t workspace_bytes, uint32_t* counts, void* stream);
int sr_mesh_filter_emit(const int32_t* faces, int32_t nv, int32_t nf, const float* vertices, const float* colors, void* workspace,
                        size_t workspace_bytes, int32_t nv_out, int32_t nf_out, float* vertices_out, float* colors_out, int32_t* faces_out,
                        void* stream);

/* The frame masks of the unveiling stage (csrc/unveil.hip): what connects the instance selection, the masked model and its losses in the
 * reference's inpainting_pipeline/ -- the point-in-frame tests of scene/__init__.py:217-312 and the pixel masks and condition images of
 * inpainting_pipeline/utils.py:17-30, 2_condition_preparation/2_generate_inpainted_mask.py:111-159 and
 * 3_reoptimization/1_optimization.py:115-187.  All pointers are device pointers; nothing is read back, nothing allocated.
 *   Cameras.  cams [F,24] float32, a row = {w2c rows 0..2 (12 values, row-major [R | t]), K (9, row-major), max_z (+inf: none),
 *     reso_scale (0: none), one unused}; hw [F,2] int32 = (h, w).  sr_points_in_frame* read one row (F = 1).
 *   The predicate, in float32, strict: cam = R x + t; p = K cam; pix = p.xy / p.z (IEEE division); a point is in the frame iff
 *     pix.x < w, pix.x > 0, pix.y < h, pix.y > 0, cam.z > 0 and cam.z < max_z.  A NaN decides nothing true; a point with a NaN or infinite
 *     coordinate is in no frame.  Pixel coordinates: trunc(pix), then trunc(trunc(pix) / reso_scale) in float32 true division where a
 *     scale is given; int64.  depth = cam.z.
 *   sr_points_in_frame: mask [P] bytes (0 / 1).  With count != NULL it also scans the flags into the workspace and leaves the number of
 *     admitted points in count[0] (DEVICE memory: the one read-back is the caller's); sr_points_in_frame_emit, with the same points,
 *     camera and workspace and that number n, writes pix [n,2] int64 = (x, y) and depth [n] in ascending point index.
 *   sr_frame_visibility: count [F] int64 and depth_sum [F] float64 (the float32 depths of the admitted points, added as doubles) over
 *     points x frames in one launch plus one fold of per-block partials; every addition's order depends on P alone.
 *   sr_semantic_mask_of_points: maps [F,Hm,Wm] uint8 labels; mask[i] = 1 iff in some frame that admits point i,
 *     (1 << label) & remain_bit != 0 at maps[f, pix.y, pix.x].  One thread per point walks the frames in order and stops once its point
 *     is set.  A label of 31 or more matches nothing (the reference shifts an int32 by it); bit 31 of remain_bit is ignored.  A pixel
 *     index outside [0,Hm) x [0,Wm) -- reso_scale and the map size disagree -- is not read, matches nothing and is counted in
 *     n_out_of_range[0] (uint64, device) for every frame the thread tested before it stopped (the reference would raise).
 *   The dilation.  out(y, x) = OR of the predicate at (y + dy, x + dx), dy and dx in [-(k / 2), k - 1 - k / 2], pixels outside the image
 *     contributing nothing: cv2.dilate with a k x k kernel of ones, the default anchor (k / 2, k / 2) and the default border as OpenCV
 *     documents them (not verified against cv2, which is not a dependency).  1 <= k <= 31.  Outputs are bytes (0 / 1) [H,W].
 *     sr_dilate_mask: the predicate is mask[y, x] != 0.  sr_instance_pixel_mask: |alpha_a - alpha_b| > threshold ([H,W] float32 each; a
 *     NaN difference is not set).  sr_refill_mask: not (sum over the C channels of |render_a - render_b| < eps) and mask != 0
 *     ([C,H,W] float32, the channels added in order; a NaN sum is set).  The undilated mask exists only as bits in the LDS.
 *   sr_inpaint_conditions: the images are [3,H,W] (renders, normal, sky) or [H,W] (alphas, depth) float32; with
 *     q(x) = trunc(clamp(255 x + 0.5, 0, 255)) in float32, a product then a sum (torchvision's save_image; a NaN gives 0):
 *     original_rgb = q(full_render + sky (1 - full_alpha)), inpainted_rgb = q(background_render + sky (1 - full_alpha)) -- the FULL alpha,
 *     as the reference --, empty_opacity = q(full_alpha - background_alpha), inpainted_depth = q(clamp(d, 0, 1)) with
 *     d = 1 / background_depth and an infinite d set to 0, inpainted_normal = q(clamp(0.5 n + 0.5, 0, 1)); uint8 in [H,W,C] layout; mask =
 *     sr_instance_pixel_mask(full_alpha, background_alpha, threshold, k).  Two launches.
 * P == 0 or F == 0 is no error: count and depth_sum are zeroed, nothing else is written.  Every call checks its arguments before its first
 * HIP call (SR_ERR_INVALID_ARGUMENT: a negative count, a NULL or misaligned pointer, H or W < 1, k outside 1..31, a NaN threshold;
 * SR_ERR_BUFFER_TOO_SMALL: a short workspace -- sr_unveil_workspace_bytes(P, F) bytes, 16-B aligned: 4 bytes a point + 16 per (frame, 2048
 * points); SR_ERR_UNSUPPORTED: H W beyond int32, H > 2 097 120 rows, W > 2^31 - 129 columns, C outside 1..16) and runs on the caller's stream.  Integer atomics only: equal inputs
 * give equal bits.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_unveil_workspace_bytes(int32_t P, int32_t F);
int sr_points_in_frame(int32_t P, const float* xyz, const float* cam, const int32_t* hw, uint8_t* mask, void* workspace,
                       size_t workspace_bytes, uint32_t* count, void* stream);
int sr_points_in_frame_emit(int32_t P, const float* xyz, const float* cam, const int32_t* hw, void* workspace, size_t workspace_bytes,
                            int32_t n, int64_t* pix, float* depth, void* stream);
int sr_frame_visibility(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, void* workspace,
                        size_t workspace_bytes, int64_t* count, double* depth_sum, void* stream);
int sr_semantic_mask_of_points(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, const uint8_t* maps,
                               int32_t Hm, int32_t Wm, uint32_t remain_bit, uint8_t* mask, uint64_t* n_out_of_range, void* stream);
int sr_dilate_mask(int32_t H, int32_t W, int32_t k, const uint8_t* mask, uint8_t* out, void* stream);
int sr_instance_pixel_mask(int32_t H, int32_t W, const float* alpha_a, const float* alpha_b, float threshold, int32_t k, uint8_t* out,
                           void* stream);
int sr_refill_mask(int32_t H, int32_t W, int32_t C, const float* render_a, const float* render_b, const uint8_t* mask, float eps,
                   int32_t k, uint8_t* out, void* stream);
int sr_inpaint_conditions(int32_t H, int32_t W, const float* full_render, const float* full_alpha, const float* background_render,
                          const float* background_alpha, const float* background_depth, const float* background_normal, const float* sky,
                          float threshold, int32_t k, uint8_t* mask, uint8_t* original_rgb, uint8_t* inpainted_rgb, uint8_t* empty_opacity,
                          uint8_t* inpainted_depth, uint8_t* inpainted_normal, void* stream);

/* LiDAR scene initialisation (csrc/voxel.hip): the semantic voxel downsample of the reference's SemanticPointCloud.voxel_down_sample
 * [REF utils/pcd_utils.py:73-142] -- one output point per occupied voxel.  All arrays are device arrays except lo (three HOST doubles);
 * points, colors, normals are [n,3] float32 or float64 (the *_f64 flags: 0 / 1), semantics [n] int32 or int64 (semantics_bytes 4 / 8) or
 * NULL.  n < 2^31.
 *   The voxel of a point, in the points' own dtype T: with v = (T)voxel_size and lo = min(points, 0) - (T)(voxel_size * 0.5) per axis (formed
 *     by the caller in T, handed over exactly in doubles), c = trunc((p - lo) / v) -- ONE IEEE subtraction and ONE IEEE division, never a
 *     product with the reciprocal -- and index = c.x + offset c.y + offset^2 c.z in int64, where the caller computes, in host float64,
 *     hi = max(points, 0) + (T)(voxel_size * 0.5) and offset = (int)((max(hi) - min(lo) + 2 voxel_size) / voxel_size).  1 <= offset < 2^21.
 *   sr_voxel_bounds: bounds [7] doubles = the minimum xyz and the maximum xyz over the rows whose three coordinates are finite, and the number
 *     of the other rows (the caller refuses a cloud that has one: the reference silently produces garbage there).
 *   sr_voxel_group: keys, stable sorts (label, then index: the library's radix sort in chained 32-bit passes, as many as offset asks
 *     for), segment heads, per-voxel member count and label statistics; counts [3] (DEVICE memory: the one read-back is the caller's) =
 *     {occupied voxels, kept voxels, labels outside 0..255}.  The label of a voxel is its most frequent label (the lowest of equally frequent
 *     ones); a voxel is KEPT iff 5 max_count >= 4 members in integers -- the reference's `1.0 * max / len < 0.8` in float32 drops the same
 *     voxels for every voxel of fewer than 2^23 members.  Without semantics every voxel is kept.  A label outside 0..255 is counted and
 *     otherwise taken modulo 256: the caller raises (the reference takes any int32, while the model shifts 1 << label).
 *   sr_voxel_emit, with the same cloud and workspace and the two counts read back: out_points / out_colors / out_normals [n_kept,3] float32 =
 *     the arithmetic means of the members (float64 sums in an order that depends on the inputs alone, sum / count in float64, rounded once
 *     to float32), out_semantics [n_kept] int32, and where not NULL out_counts [n_kept] int32 = the members and out_index [n_kept] int64 = the
 *     voxel index; rows in ascending voxel index.  A NULL attribute and its output are skipped.
 * Equal inputs give equal bits; integer atomics only.  A voxel of more than 128 members is given a wave, not a lane.  n == 0 is no error
 * (counts are zeroed, nothing else is written; sr_voxel_bounds refuses it).  Every call checks its arguments before its first HIP call
 * (SR_ERR_INVALID_ARGUMENT: a negative count, a NULL or misaligned pointer, a voxel_size that is not positive and finite, a non-finite lo,
 * counts that contradict each other; SR_ERR_BUFFER_TOO_SMALL: a short workspace -- sr_voxel_workspace_bytes(n) bytes, 16-B aligned;
 * SR_ERR_UNSUPPORTED: offset >= 2^21) and runs on the caller's stream.  Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_voxel_workspace_bytes(int32_t n);
int sr_voxel_bounds(int32_t n, const void* points, int32_t points_f64, void* workspace, size_t workspace_bytes, double* bounds, void* stream);
int sr_voxel_group(int32_t n, const void* points, int32_t points_f64, const void* semantics, int32_t semantics_bytes, const double* lo,
                   double voxel_size, int64_t offset, void* workspace, size_t workspace_bytes, uint32_t* counts, void* stream);
int sr_voxel_emit(int32_t n, const void* points, int32_t points_f64, const void* colors, int32_t colors_f64, const void* normals,
                  int32_t normals_f64, void* workspace, size_t workspace_bytes, int32_t n_voxels, int32_t n_kept, float* out_points,
                  float* out_colors, float* out_normals, int32_t* out_semantics, int32_t* out_counts, int64_t* out_index, void* stream);

/* LiDAR colouring and labelling from the camera frames (csrc/lidar_label.hip): what every dataset reader of the reference does to a sweep
 * before the voxel downsample [REF scene/dataset_readers/projection_utils.py:17-104, waymo.py:79-192, kitti.py:117-163,
 * pandaset.py:53-106].  One record of the DEVICE table a call reads (`views`: n_views records, 8-B aligned); it never crosses the call
 * boundary by value, so it is a plain struct tag, and streetunveiler_amd/lidar_label.py states the same 192 bytes as a numpy dtype:
 * rows 0..2 of the world-to-camera matrix (its last row must be (0, 0, 0, 1): the caller checks), the intrinsics row-major, the picture's
 * size, the picture (uint8 [h,w,3], NULL where only labels are asked for: the colour sums are then zero) and the label map (uint8 [h,w]).
 * Both pictures are dense and have EXACTLY h x w pixels: the library cannot check device memory and reads pixel (v, u) at v * w + u. */
struct SrLabelView {
    double w2c[12];
    double K[9];
    int32_t h, w;
    const uint8_t* image;
    const uint8_t* map;
};
/*   The predicate, in float64 in this order whatever the points' dtype (float32 is widened on load), no fused operation:
 *     cam_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i,  p_i = (K_i0 cam_0 + K_i1 cam_1) + K_i2 cam_2,  pix = (p_0 / p_2, p_1 / p_2) by IEEE division;
 *     inside iff pix.x < w && pix.x > 0 && pix.y < h && pix.y > 0 && cam_2 > 0 -- all strict, false for a NaN -- and x, y, z are finite;
 *     (u, v) = trunc(pix).
 *   The certainty test with r = check_range >= 0 and l0 = lut[map[v,u]] (label_lut: 256 device bytes applied to every map byte as it is
 *     read, NULL = identity): the corners (v-r, u-r), (v-r, u+r), (v+r, u-r) and the fourth are compared with l0 where they are valid --
 *     v-r > 0 resp. v+r < h with u-r > 0 resp. u+r < w, so row 0 and column 0 never are -- and the point is certain when no valid corner
 *     differs.  fourth_corner = 0 (the reference): the fourth corner, valid when v+r < h && u+r < w, reads COLUMN u-r, which wraps to
 *     w + u - r where it is negative (the reference's own line 94 under numpy's indexing); 1 (mirrored): it reads (v+r, u+r).
 *   sr_lidar_label_decide: sweep s = the points sweep_offsets[s] .. sweep_offsets[s+1] (DEVICE int32 [n_sweeps + 1], ascending from 0 to n;
 *     values outside are clamped, max_sweep_points >= the longest sweep) goes through the views s C .. s C + C - 1, C = cameras_per_sweep in
 *     1..32, n_views >= n_sweeps C, n_views <= 65535.  per_view = 0: one row a point -- over its sweep's cameras in order, where the point is
 *     inside and certain, the pixel's three bytes are added to integer sums, 1 to its count and label = lut[map[v,u]] (the last camera wins);
 *     rows with count > 0 are kept.  per_view = 1: one row per (point, camera) that is inside and certain, in the order (sweep, camera,
 *     point); n C < 2^31.  Rows and their scanned output offsets stay in the workspace; counts [2] (DEVICE uint64; the one read-back is
 *     the caller's) = {kept rows, 0}.
 *   sr_lidar_vote: every point through every view, no certainty test: per point the hits per class lut[map[v,u]] < n_classes (1..8) and
 *     whether any view saw it -> valid_mask [n] bytes; a point's row carries tag = the FIRST largest class (argmax), count 1 where valid.
 *     counts = {valid points, (point, view) hits whose label >= n_classes -- counted, not added to a class: the caller raises}.
 *   sr_lidar_label_emit, after either on the same points, offsets and workspace, rows_per_point = 1 (per_view = 0, the vote) or C, n_rows =
 *     counts[0]: out_xyz [n_rows,3] in the points' dtype, bit for bit; out_rgb [n_rows,3] doubles = sums / count, one IEEE division of
 *     exact integers, on the 0..255 scale; out_semantics int32, out_index int64 = the point's index; rows_per_sweep int32 [n_sweeps].
 *     NULL outputs are skipped; sweep_offsets NULL = one sweep of all points.
 * Equal inputs give equal bits: the order comes from a prefix sum, the only atomic is the integer counter of the vote.  Every call checks its
 * host arguments before its first HIP call and runs on the caller's stream; n == 0 is no error (counts are zeroed).  n < 2^31.
 * Added without a new SR_ABI_VERSION: nothing that existed changed. */
size_t sr_lidar_label_workspace_bytes(int32_t n, int32_t rows_per_point);
int sr_lidar_label_decide(int32_t n, const void* points, int32_t points_f64, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points,
                          const void* views, int32_t n_views, int32_t cameras_per_sweep, int32_t check_range, int32_t fourth_corner,
                          const uint8_t* label_lut, int32_t per_view, void* workspace, size_t workspace_bytes, uint64_t* counts, void* stream);
int sr_lidar_label_emit(int32_t n, const void* points, int32_t points_f64, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points,
                        int32_t rows_per_point, void* workspace, size_t workspace_bytes, int32_t n_rows, void* out_xyz, double* out_rgb,
                        int32_t* out_semantics, int64_t* out_index, int32_t* rows_per_sweep, void* stream);
int sr_lidar_vote(int32_t n, const void* points, int32_t points_f64, const void* views, int32_t n_views, int32_t n_classes, const uint8_t* label_lut,
                  void* workspace, size_t workspace_bytes, uint8_t* valid_mask, uint64_t* counts, void* stream);

/* Frame resizing with Pillow's 8-bit arithmetic, and nearest label maps (csrc/resize.hip): how a camera frame, an inpainted frame and a
 * label map reach the training resolution [REF utils/camera_utils.py:22-73, utils/general_utils.py:21-27,
 * inpainting_pipeline/3_reoptimization/1_optimization.py:140-199] -- Image.resize(size, BICUBIC or BILINEAR) of an "L" or "RGB" image bit
 * for bit, and transforms.Resize(NEAREST) of a label tensor.  All pointers are device pointers and both calls CHECK that (an address the
 * HIP runtime does not know as device or managed memory is refused); nothing is read back, nothing allocated.
 *   A frame is N pictures of H x W pixels of C = 1 or 3 dense bytes; a row's pixels are dense, row y of picture n starts at byte
 *     n in_batch_stride + y in_row_stride (in_row_stride >= W C, in_batch_stride >= 0; sr_resize_nearest: the same in ELEMENTS, C = 1).
 *   sr_resize_u8_pass: ONE pass of the separable resize.  axis 0 resamples the columns (W -> out_size, the output is [N,H,out_size,C]),
 *     axis 1 the rows (H -> out_size, [N,out_size,W,C]), axis -1 neither (out_size, bounds, coeffs and ksize are ignored).  For output
 *     index o: first = bounds[2 o], count = bounds[2 o + 1] (int32 [out_size,2]), k = coeffs + o ksize (int32 [out_size,ksize]) and
 *       v = clamp((2^21 + sum over i < count of in[first + i] k[i]) >> 22, 0, 255)
 *     with a 32-bit wrapping sum and an arithmetic shift.  first is clamped into [0, in_size] and count into [0, min(ksize, in_size -
 *     first)] before anything is read: no table reads outside the picture.  The tables are the caller's (Pillow's precompute_coeffs and
 *     normalize_coeffs_8bpc in host float64; streetunveiler_amd.frames.resize_tables); the loop runs to count, whatever ksize is.
 *     A resize is axis 0, then axis 1 on its uint8 output; a pass whose axis keeps its size is left out; a resize that changes neither is
 *     axis -1 (a copy).  flags, the epilogue of the LAST pass of a resize: 0 = out is uint8 [N,h,w,C]; SR_RESIZE_BINARISE = uint8, 255
 *     where v > 0, else 0; SR_RESIZE_F32_CHW = out is float32 [N,C,h,w] holding v / 255.0f by IEEE division (not a product with a
 *     reciprocal).
 *   sr_resize_nearest: out[n, y, x] = in[n, min(floor(y sy), H - 1), min(floor(x sx), W - 1)] with sy = float32(H) / float32(h), sx
 *     likewise and the products in float32 -- F.interpolate(mode="nearest").  elem_bytes = 1, 4 or 8 (uint8, int32, int64: the elements
 *     are copied as they are); out is dense [N,h,w].
 * Every call checks its arguments before its first launch (SR_ERR_INVALID_ARGUMENT: N, H, W, out_size, h, w or ksize < 1, an axis outside
 * -1..1, unknown flag bits, SR_RESIZE_BINARISE together with SR_RESIZE_F32_CHW, a NULL, misaligned or HOST pointer -- "in is not device
 * memory (a host address?)" --, out == in, a row stride below a dense row, a negative batch stride; SR_ERR_UNSUPPORTED: C other than 1 or
 * 3 -- Pillow resizes an alpha channel through premultiplied alpha, which is not built --, elem_bytes other than 1, 4, 8, a size above
 * 2^24, more than 262 140 output rows, more than 65535 pictures (x C for the float output) a call) and runs on the caller's stream.
 * Integers throughout but for the one division: equal inputs give equal bits.  Added without a new SR_ABI_VERSION: nothing that existed
 * changed. */
#define SR_RESIZE_BINARISE 1u
#define SR_RESIZE_F32_CHW 2u
int sr_resize_u8_pass(int32_t N, int32_t H, int32_t W, int32_t C, const uint8_t* in, int64_t in_batch_stride, int64_t in_row_stride,
                      int32_t axis, int32_t out_size, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, uint32_t flags, void* out,
                      void* stream);
int sr_resize_nearest(int32_t N, int32_t H, int32_t W, int32_t elem_bytes, const void* in, int64_t in_batch_stride, int64_t in_row_stride,
                      int32_t h, int32_t w, void* out, void* stream);

/* Test hook of the parity bars: the hard decisions the blend kernels take, dumped per (list entry, pixel) pair.  For list position
 * j (index into SrBinningView.point_list) and 8x8 quadrant q of its tile (q = (y / 8) * (tile_width / 8) + x / 8, bit = (y % 8) * 8 + x % 8
 * in tile-local pixel coordinates): valid_bits[j * nq + q] = pixels where the entry passes the chain of skips of the forward blend
 * (p.z != 0, depth >= near, power <= 0, alpha >= 1/255 -- NOT the pixel's saturation state), use3d_bits = pixels where it takes the
 * ray-splat path (rho3d <= rho2d).  Computed by the same device functions on the same staged values as K6 / K7, i.e. these are the
 * bits they act on; tests/ hands them to the CPU oracle so that both sides blend the same contributor sets.
 * Both arrays: device [num_rendered * nq] u64, nq = (tile_width / 8) * (tile_height / 8). */
int sr_debug_pair_decisions(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning,
                            size_t binning_bytes, uint32_t num_rendered, uint64_t* valid_bits, uint64_t* use3d_bits, void* stream);

/* Test hook for the library's stable LSD radix sort (binning K2/K4): sorts n (key, value) u32 pairs by key bits
 * [0, total_bits); vals_in == NULL means value = index.  temp: sr_debug_radix_sort_temp_bytes(n) bytes. */
size_t sr_debug_radix_sort_temp_bytes(uint32_t n);
int sr_debug_radix_sort(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t n,
                        int total_bits, void* temp, size_t temp_bytes, uint32_t flags /* SR_FLAG_BALLOT_RANKING or 0 */, void* stream);

/* How the sort / partition kernels of the current device rank items (the run-time guard of the LDS-atomic lane-order assumption):
 * runs the self-check on first use (one tiny kernel + one stream wait per device and process), then returns the cached answer:
 * 1 = LDS-atomic return values (the property holds), 2 = match-any ballots (it does not: the fallback is in use), or
 * SR_ERR_UNSUPPORTED if neither ranking reproduces the reference ranks on this device. */
int sr_rank_mode(void* stream);

/* Test hook for the hardware property the sort kernels rank by: within one wave instruction, ds_add_rtn_u32 returns the old values
 * to the lanes that hit the same LDS address in ascending lane order.  ranks[i] = what lane i % 64 of its wave got back when every
 * lane added 1 to counter digits[i] % bins of its wave (n a multiple of 256, processed 256 per block step, 8 steps per block, the
 * counters running on across the steps; bins <= 1024).  All device pointers. */
int sr_debug_lds_atomic_ranks(const uint32_t* digits, uint32_t* ranks, uint32_t n, int bins, void* stream);

/* Profiling aid -- the one piece of process-wide state in this library (mutex-protected: autograd runs the backward on its own
 * thread).  sr_set_stage_timing(1) makes every later call bracket each stage with a pair of HIP events recorded
 * on the caller's stream (no host sync while recording; up to 512 launches per stage); sr_set_stage_timing(2 * mask),
 * mask = OR of (1 << SrStage), brackets only the stages in the mask (every event pair costs a few microseconds of
 * stream time: the full set adds ~1.4 % to a 4.5 ms step).  sr_stage_stats() waits for the recorded events and returns the
 * summed duration (ms) and the number of launches of one stage since timing was (re-)enabled. */
typedef enum SrStage {
    SR_STAGE_PREPROCESS = 0, SR_STAGE_DEPTH_SORT = 1, SR_STAGE_SCAN = 2, SR_STAGE_EXPAND_X = 3, SR_STAGE_EXPAND_Y = 4,
    SR_STAGE_RANGES = 5, SR_STAGE_BLEND_FWD = 6, SR_STAGE_BLEND_BWD = 7, SR_STAGE_PREPROCESS_BWD = 8,
    /* the per-class distortion pass's own kernels (its K1..K5 and K8 are the stages above) */
    SR_STAGE_CLASS_PARTITION = 9, SR_STAGE_CLASS_FWD = 10, SR_STAGE_CLASS_BWD = 11, SR_STAGE_COUNT = 12
} SrStage;
void sr_set_stage_timing(int enable);
int sr_stage_stats(int stage, float* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* SURFEL_RASTER_H */
