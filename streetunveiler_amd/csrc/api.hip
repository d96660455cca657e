// api.hip -- the C-ABI (include/surfel_raster.h): buffer layouts, argument checks, stage sequencing.
// No torch types, no exceptions across the boundary, nothing allocated persistently.
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <atomic>
#include <mutex>

#include "launch.h"

using namespace sr;

namespace {

thread_local char g_err[512] = "";
// The only process-wide state of the library is this profiling aid (everything that changes what a call does is a field
// of that call's SrFrame): autograd runs the backward on its own thread, so the rings are shared and mutex-protected.
std::atomic<int> g_timing{0};
std::mutex g_ring_mu;

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define SR_HIP(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return fail(SR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                               \
    } while (0)

// Stage timing: a ring of HIP event pairs per stage, recorded on the caller's stream (no sync while
// recording); sr_stage_stats() synchronises on the recorded events and returns total ms + launch count.
constexpr int kEvRing = 512;
struct EvRing {
    hipEvent_t ev[kEvRing][2];
    bool closed[kEvRing];   // the end event of the slot has been recorded (a reader skips a pair whose timer is still open)
    int created = 0, used = 0;
};
EvRing g_ring[SR_STAGE_COUNT];

struct StageTimer {
    int stage; hipStream_t s; int slot = -1;
    StageTimer(int st, hipStream_t stream) : stage(st), s(stream) {
        const int mode = g_timing.load();   // 0 off, 1 every stage, otherwise a bit mask of stages (bit 1 << stage, shifted by one)
        if (!mode || (mode != 1 && !((mode >> 1) & (1 << stage)))) return;
        std::lock_guard<std::mutex> lk(g_ring_mu);
        EvRing& r = g_ring[stage];
        if (r.used >= kEvRing) return;  // ring full: stop recording (stats stay valid for the recorded part)
        if (r.used >= r.created) {
            if (hipEventCreate(&r.ev[r.created][0]) != hipSuccess || hipEventCreate(&r.ev[r.created][1]) != hipSuccess) return;
            ++r.created;
        }
        slot = r.used++;   // reserved here: a timer started meanwhile on another thread (autograd's backward) gets the next one
        r.closed[slot] = false;
        (void)hipEventRecord(r.ev[slot][0], s);   // (two records per stage: each costs ~5 us of stream time)
    }
    ~StageTimer() {
        if (slot < 0) return;
        std::lock_guard<std::mutex> lk(g_ring_mu);
        if (hipEventRecord(g_ring[stage].ev[slot][1], s) == hipSuccess) g_ring[stage].closed[slot] = true;
    }
};

int debug_sync(const SrFrame* frame, hipStream_t s, const char* what) {
    if (!frame->debug) return SR_OK;
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(SR_ERR_HIP, "[debug] after %s: %s", what, hipGetErrorString(e));
    return SR_OK;
}

// One 64-B pinned host block per calling thread (with one event per (thread, device) the only things this library keeps): word 0 =
// the DMA target of the num_rendered read-back, words 4..7 = the four counts of sr_densify_plan, word 8 = the result word of the rank
// self-check.
// (portable + mapped: valid on every device of the process, whichever is current when the thread first calls in.  Never freed: 64 B per
// calling thread, and a destructor at thread / process exit could run after the HIP runtime has been torn down.)
uint32_t* pinned_words() {
    static thread_local uint32_t* pinned = nullptr;
    if (!pinned && hipHostMalloc(reinterpret_cast<void**>(&pinned), 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { pinned = nullptr; (void)hipGetLastError(); }
    return pinned;
}

// The device a stream belongs to (the cache below is per device: the CURRENT device may be another one); the null stream -> current device.
int stream_device(hipStream_t s, int* dev) {
    hipDevice_t d = 0;
    if (s && hipStreamGetDevice(s, &d) == hipSuccess) { *dev = (int)d; return SR_OK; }
    (void)hipGetLastError();
    SR_HIP(hipGetDevice(dev));
    return SR_OK;
}

// How the sort / partition kernels rank items inside a wave (common.h take_run_slot).  The fast path relies on the lane order of LDS
// atomic returns, which gfx950 delivers but no document promises -- so the first call on every device runs rank_selfcheck_kernel
// (~20 us) and the answer is cached per device for the life of the process: kRankAtomic, else the match-any ballots (kRankBallot),
// else nothing this library can sort with (SR_ERR_UNSUPPORTED).  SR_FLAG_BALLOT_RANKING forces the ballots for one call.
constexpr int kMaxDevices = 64;
std::atomic<int> g_rank_mode[kMaxDevices];
int rank_mode(hipStream_t s, bool force_ballot, RankMode* mode) {
    int dev = 0;
    { const int rc = stream_device(s, &dev); if (rc != SR_OK) return rc; }
    if (dev < 0 || dev >= kMaxDevices) return fail(SR_ERR_UNSUPPORTED, "device index %d beyond %d", dev, kMaxDevices);
    int m = g_rank_mode[dev].load(std::memory_order_acquire);
    if (m == kRankUnknown) {
        // the self-check waits on the stream: not possible while the stream is being captured into a graph -- warm up first
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
            return fail(SR_ERR_UNSUPPORTED, "the stream is capturing and device %d has not run the rank self-check yet: call sr_rank_mode(stream) once before the capture", dev);
        (void)hipGetLastError();
        struct Scratch { uint32_t* p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } } scratch;   // freed on every path out of here
        uint32_t* host = pinned_words();
        uint32_t* result = nullptr;
        const bool temp = !(host && hipHostGetDevicePointer(reinterpret_cast<void**>(&result), host + 8, 0) == hipSuccess && result);
        if (!temp) host[8] = 0;
        else { (void)hipGetLastError(); SR_HIP(hipMalloc(reinterpret_cast<void**>(&scratch.p), 4)); result = scratch.p; SR_HIP(hipMemsetAsync(result, 0, 4, s)); }
        SR_HIP(launch_rank_selfcheck(result, s));
        uint32_t r = 0;
        if (temp) { SR_HIP(hipMemcpyAsync(&r, result, 4, hipMemcpyDeviceToHost, s)); SR_HIP(hipStreamSynchronize(s)); }
        else { SR_HIP(hipStreamSynchronize(s)); r = *reinterpret_cast<volatile uint32_t*>(host + 8); }
        if (!(r & 0x100u)) return fail(SR_ERR_HIP, "the rank self-check kernel did not report back");
        m = (r & 1u) ? kRankAtomic : ((r & 2u) ? kRankBallot : kRankNone);
        g_rank_mode[dev].store(m, std::memory_order_release);
    }
    if (m == kRankNone) return fail(SR_ERR_UNSUPPORTED, "neither LDS-atomic nor ballot ranking passes the self-check on device %d", dev);
    *mode = force_ballot ? kRankBallot : static_cast<RankMode>(m);
    return SR_OK;
}

// ---- buffer layouts ------------------------------------------------------------------------------
// A layout = the byte offsets of a state buffer's regions (every region 256-B aligned) + its total; a view = the typed pointers of one
// buffer carved by that layout.  Every entry point carves once, through these (launch.h: Carver, at<T>).
constexpr int kMaxTilesPerAxis = SR_MAX_TILES_PER_AXIS;   // binning.hip kXpMaxBins: 10-bit row / column fields, 1024-entry LDS histograms

struct GeomLayout {
    size_t recs, depth_keys, tiles_touched, rect, clamped, sorted_keys, sorted_gid, rect_sorted, first, sh_jac, block_base, base_bytes,
        counts, temp, temp_bytes, total;
};
GeomLayout geom_layout(int P) {
    GeomLayout L{};
    const size_t n = (size_t)(P > 0 ? P : 1);
    Carver c;
    L.recs = c.take(n * kRecFloats * 4);
    L.depth_keys = c.take(n * 4);
    L.tiles_touched = c.take(n * 4);
    L.rect = c.take(n * 8);
    L.clamped = c.take(n);
    L.sorted_keys = c.take(n * 4);
    L.sorted_gid = c.take(n * 4);
    L.rect_sorted = c.take(n * 8);
    L.first = c.take(n * 4);
    L.sh_jac = c.take(n * 36);
    L.base_bytes = tile_scan_temp_bytes(P);
    L.block_base = c.take(L.base_bytes);
    const size_t n_scan_blocks = (n + 2047) / 2048;   // the scan's block size (radix_sort.hip kRsTile)
    L.counts = L.block_base + n_scan_blocks * 4;      // the frame's count words follow the block bases: GeomView::counts
    static thread_local int memo_P = -1;
    static thread_local size_t memo_bytes = 0;
    if (memo_P != P) {   // the depth sort's ping-pong + histogram; later pass X's [tile columns][blocks] histogram (any frame width)
        memo_bytes = depth_sort_temp_bytes(P);
        const size_t hx = align_up(expand_x_hist_bytes(P, kMaxTilesPerAxis), 256);
        if (hx > memo_bytes) memo_bytes = hx;
        memo_P = P;
    }
    L.temp_bytes = memo_bytes;
    L.temp = c.take(L.temp_bytes);
    L.total = c.off;
    return L;
}
// The words of GeomView::counts (SrGeomView.frame_counts), left by the emission scan.  (kCountOverflow is a per-block count the scan is done
// with by the time the capacity guard writes it.)
enum FrameCount { kCountDuplicates = 0, kCountVisible = 1, kCountOverflow = 2 };
struct GeomView {
    float4* recs; uint32_t* depth_keys; uint32_t* tiles_touched; uint2* rect; uint8_t* clamped;
    uint32_t* sorted_keys; uint32_t* sorted_gid; uint2* rect_sorted; uint32_t* first;
    float* sh_jac;          // (the stand-alone class pass keeps its class id bytes here: it has no SH colour)
    uint32_t* block_base; void* temp;
    uint32_t* counts;       // [FrameCount]
};
GeomView geom_view(void* geom, const GeomLayout& L) {
    return GeomView{at<float4>(geom, L.recs), at<uint32_t>(geom, L.depth_keys), at<uint32_t>(geom, L.tiles_touched), at<uint2>(geom, L.rect),
                    at<uint8_t>(geom, L.clamped), at<uint32_t>(geom, L.sorted_keys), at<uint32_t>(geom, L.sorted_gid), at<uint2>(geom, L.rect_sorted),
                    at<uint32_t>(geom, L.first), at<float>(geom, L.sh_jac), at<uint32_t>(geom, L.block_base), at<void>(geom, L.temp),
                    at<uint32_t>(geom, L.counts)};
}

struct BinLayout {
    size_t columns, point_list, hit_mask, ranges, order, tile_counts, row_total, n_columns, hist, hist_bytes, total;
};
BinLayout bin_layout(uint32_t D, int W, int H) {
    BinLayout L{};
    const size_t n = (size_t)(D > 0 ? D : 1);
    const int tiles = ((W + 7) / 8) * ((H + 7) / 8);   // sized for the smallest tile shape (8x8); the reference's 16x16 uses a quarter
    Carver c;
    L.columns = c.take(n * 8);   // column items of the expanding partition: at most D of them
    L.point_list = c.take(n * 4);
    L.hit_mask = c.take(n * 2);
    L.ranges = c.take((size_t)(tiles > 0 ? tiles : 1) * 8);
    L.order = c.take((size_t)(tiles > 0 ? tiles : 1) * 4);
    L.tile_counts = c.take((size_t)(tiles > 0 ? tiles : 1) * 4);
    L.row_total = c.take((size_t)kMaxTilesPerAxis * 4);
    L.n_columns = c.take(4);
    L.hist_bytes = expand_y_hist_bytes(D, (H + 7) / 8);
    L.hist = c.take(L.hist_bytes);
    L.total = c.off;
    return L;
}
struct BinView {
    uint2* columns;          // (dead once pass Y has run: the class passes keep their class-ordered tile lists here, as uint32_t)
    uint32_t* point_list; uint16_t* hit_mask; uint2* ranges; uint32_t* order; uint32_t* tile_counts; uint32_t* row_total; uint32_t* n_columns; uint32_t* hist;
    uint32_t* class_list() const { return reinterpret_cast<uint32_t*>(columns); }
};
BinView bin_view(void* binning, const BinLayout& L) {
    return BinView{at<uint2>(binning, L.columns), at<uint32_t>(binning, L.point_list), at<uint16_t>(binning, L.hit_mask), at<uint2>(binning, L.ranges),
                   at<uint32_t>(binning, L.order), at<uint32_t>(binning, L.tile_counts), at<uint32_t>(binning, L.row_total), at<uint32_t>(binning, L.n_columns),
                   at<uint32_t>(binning, L.hist)};
}

struct ImgLayout { size_t final_T, n_contrib, total; };
ImgLayout img_layout(int W, int H) {
    ImgLayout L{};
    const size_t hw = (size_t)(W > 0 ? W : 1) * (size_t)(H > 0 ? H : 1);
    Carver c;
    L.final_T = c.take(hw * 3 * 4);
    L.n_contrib = c.take(hw * 2 * 4);
    L.total = c.off;
    return L;
}
struct ImgView { float* final_T; uint32_t* n_contrib; };
ImgView img_view(void* image, const ImgLayout& L) { return ImgView{at<float>(image, L.final_T), at<uint32_t>(image, L.n_contrib)}; }

// The backward workspace: one gradient record (96 B; 112 B with 9 colour channels) + one `written` byte per (tile, Gaussian) duplicate, in
// emission order (a Gaussian's duplicates are contiguous).  K7 writes a record -- and sets the slot's byte in `written` -- only where some
// pixel contributed; K8 looks at the byte before it touches the record, so neither the records nor anything but these D bytes need clearing.
size_t record_bytes(int color_channels) { return (size_t)(color_channels == 9 ? kGradFloats + 4 : kGradFloats) * 4; }
struct WorkspaceLayout { size_t records, written, total; };
WorkspaceLayout workspace_layout(uint32_t D, int color_channels) {
    const size_t n = (size_t)(D > 0 ? D : 1);
    WorkspaceLayout L{};
    Carver c;
    L.records = c.take(n * record_bytes(color_channels));
    L.written = c.take(n);
    L.total = c.off;
    return L;
}
struct WorkspaceView { float4* records; uint8_t* written; };
WorkspaceView workspace_view(void* workspace, uint32_t D, int color_channels) {
    const WorkspaceLayout L = workspace_layout(D, color_channels);
    return WorkspaceView{at<float4>(workspace, L.records), at<uint8_t>(workspace, L.written)};
}

struct TileShape { int w, h; };
TileShape tile_shape(const SrFrame* frame) {   // (0 = the reference's 16x16)
    return TileShape{frame->tile_width > 0 ? frame->tile_width : kTile, frame->tile_height > 0 ? frame->tile_height : kTile};
}

int check_common(const SrFrame* frame, const SrGaussians* g) {
    if (!frame || !g) return fail(SR_ERR_INVALID_ARGUMENT, "frame / gaussians is NULL");
    if (frame->image_width <= 0 || frame->image_height <= 0) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", frame->image_width, frame->image_height);
    if (g->P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    {
        const TileShape t = tile_shape(frame);
        const bool known = (t.w == 16 && t.h == 16) || (t.w == 8 && t.h == 8) || (t.w == 16 && t.h == 8) || (t.w == 32 && t.h == 8) || (t.w == 32 && t.h == 16);
        if (!known) return fail(SR_ERR_UNSUPPORTED, "tile shape %dx%d not in {8x8, 16x8, 16x16, 32x8, 32x16}", t.w, t.h);
    }
    if (!frame->bg || !frame->viewmatrix || !frame->projmatrix || !frame->campos) return fail(SR_ERR_INVALID_ARGUMENT, "bg / viewmatrix / projmatrix / campos must be non-NULL device pointers");
    if (g->P > 0) {
        if (!g->means3D || !g->opacities) return fail(SR_ERR_INVALID_ARGUMENT, "means3D / opacities is NULL");
        if (g->color_channels == 9) {   // SH colour + six precomputed channels in one pass
            if (!g->shs || !g->colors_precomp) return fail(SR_ERR_INVALID_ARGUMENT, "9 colour channels need SHs AND a [P,6] precomputed colour array");
        } else if ((g->shs != nullptr) == (g->colors_precomp != nullptr)) return fail(SR_ERR_INVALID_ARGUMENT, "Please provide exactly one of either SHs or precomputed colors!");
        if (g->color_channels != 0 && g->color_channels != 3 && g->color_channels != 6 && g->color_channels != 9) return fail(SR_ERR_UNSUPPORTED, "color_channels %d not in {3, 6, 9}", g->color_channels);
        if (g->activations & ~(SR_ACT_EXP_SCALES | SR_ACT_SIGMOID_OPACITY | SR_ACT_NORMALIZE_ROTATIONS)) return fail(SR_ERR_UNSUPPORTED, "unknown activation bits 0x%x", g->activations);
        if (g->color_channels == 6 && g->shs) return fail(SR_ERR_INVALID_ARGUMENT, "6 colour channels need precomputed colors, not SHs");
        const bool sr_pair = g->scales != nullptr && g->rotations != nullptr;
        if ((g->scales != nullptr) != (g->rotations != nullptr) || sr_pair == (g->transMat_precomp != nullptr))
            return fail(SR_ERR_INVALID_ARGUMENT, "Please provide exactly one of either scale/rotation pair or precomputed transMat!");
        if (g->shs) {
            if (frame->sh_degree < 0 || frame->sh_degree > 3) return fail(SR_ERR_UNSUPPORTED, "sh_degree %d not in 0..3", frame->sh_degree);
            if (g->sh_coeffs < (frame->sh_degree + 1) * (frame->sh_degree + 1)) return fail(SR_ERR_INVALID_ARGUMENT, "shs has %d coefficients, degree %d needs %d", g->sh_coeffs, frame->sh_degree, (frame->sh_degree + 1) * (frame->sh_degree + 1));
        }
    }
    return SR_OK;
}

// The backward entry points read SrFrame.tanfovx / tanfovy (upstream's backward derives the image size from them: SR_BACKWARD_WH_FROM_FOCAL, the
// shipped default; the forward never did): a caller that left them 0 or NaN would get inf * 0 = NaN, (int)NaN -- undefined behaviour -- and
// a silently wrong viewport chain in K8.
int check_backward_frame(const SrFrame* frame) {
#if SR_BACKWARD_WH_FROM_FOCAL
    if (!(frame->tanfovx > 0.f) || !(frame->tanfovy > 0.f) || !std::isfinite(frame->tanfovx) || !std::isfinite(frame->tanfovy))
        return fail(SR_ERR_INVALID_ARGUMENT, "tanfovx / tanfovy must be finite and > 0 for a backward call (got %g, %g)", (double)frame->tanfovx, (double)frame->tanfovy);
#else
    (void)frame;
#endif
    return SR_OK;
}

FrameDev make_frame(const SrFrame* frame, const SrGaussians* g) {
    FrameDev f{};
    f.W = frame->image_width; f.H = frame->image_height;
    f.bw_W = f.W; f.bw_H = f.H;
#if SR_BACKWARD_WH_FROM_FOCAL
    if (frame->tanfovx > 0.f && frame->tanfovy > 0.f && std::isfinite(frame->tanfovx) && std::isfinite(frame->tanfovy)) {
        // upstream's backward: focal = size / (2 tanfov) (rasterizer_impl), then W = int(focal_x * tan_fovx * 2) in float32
        // (a forward call may leave the two fields unset -- it never reads bw_W / bw_H; the backward entry points insist: check_backward_frame)
        const float focal_x = (float)f.W / (2.0f * frame->tanfovx), focal_y = (float)f.H / (2.0f * frame->tanfovy);
        f.bw_W = (int)(focal_x * frame->tanfovx * 2); f.bw_H = (int)(focal_y * frame->tanfovy * 2);
    }
#endif
    const TileShape t = tile_shape(frame);
    f.tile_w = t.w; f.tile_h = t.h;
    f.inv_tile_w = 1.f / (float)f.tile_w; f.inv_tile_h = 1.f / (float)f.tile_h;
    f.tiles_x = (f.W + f.tile_w - 1) / f.tile_w; f.tiles_y = (f.H + f.tile_h - 1) / f.tile_h;
    f.sh_degree = frame->sh_degree; f.sh_coeffs = g->sh_coeffs;
    f.colors = g->color_channels == 6 ? 6 : (g->color_channels == 9 ? 9 : 3);
    f.activations = g->activations;
    f.scale_modifier = frame->scale_modifier;
    f.bg = frame->bg; f.view = frame->viewmatrix; f.proj = frame->projmatrix; f.campos = frame->campos;
    f.overflow = nullptr;   // (set by the backward entry points in capacity mode)
    return f;
}
// what the per-Gaussian backward kernels read of the geometry state
void set_backward_state(FrameDev* f, const SrFrame* frame, const GeomView& G) {
    f->first = G.first; f->first_base = G.block_base; f->sh_jac = G.sh_jac;
    if (frame->flags & SR_FLAG_BINNING_CAPACITY) f->overflow = G.counts + kCountOverflow;
}

// The blend PAIR of a frame: which forward kernel, which backward kernel, and the hit-mask format the two share.  The forward and the
// backward of one frame carry the same flags (include/surfel_raster.h) and both come through here, so they cannot disagree on the format
// (a row-mapped backward on quadrant masks computed silently wrong gradients).  Only the 16x16 tile with three colour channels has a choice:
//
//   public flags (16x16, 3 channels)                 forward kernel                           backward kernel          hit masks
//   blend_counters                                   kCounting                                as the pair flag says    per quadrant
//   SR_FLAG_ROW_BACKWARD                             kRowsCellMasks                           kRows                    per 4x4 cell
//   SR_FLAG_COOP_BACKWARD, culling on, no mapping    kCoop                                    kCoop                    per quadrant
//   SR_FLAG_COOP_BACKWARD otherwise                  as without it                            kCoop                    per quadrant
//   SR_FLAG_ONE_WAVE_BACKWARD                        as without it                            kOneWave                 per quadrant
//   none of the three pair flags                     SR_FLAG_ROW_MAPPED_FORWARD: kRows        kByTileCount             per quadrant
//                                                    SR_FLAG_QUADRANT_MAPPED_FORWARD or
//                                                    SR_FLAG_NO_QUADRANT_CULL: kQuadrantBands
//                                                    else: kDevicePicked
//   every other tile shape / channel count           its one kernel (kCounting: 16x16 x 6)    kOneWave                 per quadrant
//
// Refused: two of the three pair flags; both mapping flags; SR_FLAG_ROW_MAPPED_FORWARD or SR_FLAG_ROW_BACKWARD off the 16x16 tile, with other
// than three channels or with SR_FLAG_NO_QUADRANT_CULL -- and, in the forward call, with blend_counters; SR_FLAG_ROW_BACKWARD in a forward
// call with SR_FLAG_QUADRANT_MAPPED_FORWARD or SR_FLAG_FORWARD_ONLY; blend_counters off 16x16 x {3, 6} or with SR_FLAG_FORWARD_ONLY.
// `forward_call`: the preconditions of the forward-only flags (mapping, counters, forward-only) bind the forward call alone -- a backward
// call does not read those flags.
int choose_blend(const SrFrame* frame, const FrameDev& f, bool forward_call, BlendChoice* out) {
    const uint32_t flags = frame->flags;
    const uint32_t pair = flags & (SR_FLAG_ONE_WAVE_BACKWARD | SR_FLAG_COOP_BACKWARD | SR_FLAG_ROW_BACKWARD);
    if (pair & (pair - 1))
        return fail(SR_ERR_INVALID_ARGUMENT, "SR_FLAG_ONE_WAVE_BACKWARD, SR_FLAG_COOP_BACKWARD and SR_FLAG_ROW_BACKWARD exclude each other (flags 0x%x)", pair);
    const bool reference = f.tile_w == 16 && f.tile_h == 16 && f.colors == 3;   // the reference's tile, three colour channels
    const bool cull = !(flags & SR_FLAG_NO_QUADRANT_CULL), counters = forward_call && frame->blend_counters != nullptr;
    const bool rows = forward_call && (flags & SR_FLAG_ROW_MAPPED_FORWARD), quads = forward_call && (flags & SR_FLAG_QUADRANT_MAPPED_FORWARD);
    const bool fwd_only = forward_call && (flags & SR_FLAG_FORWARD_ONLY);
    if (fwd_only && counters) return fail(SR_ERR_UNSUPPORTED, "SR_FLAG_FORWARD_ONLY and blend_counters exclude each other");
    if (counters && !(f.tile_w == 16 && f.tile_h == 16 && (f.colors == 3 || f.colors == 6)))
        return fail(SR_ERR_UNSUPPORTED, "blend_counters: the counting variant of the forward blend exists for the 16x16 tile with 3 or 6 colour channels only");
    if (rows && quads) return fail(SR_ERR_INVALID_ARGUMENT, "SR_FLAG_ROW_MAPPED_FORWARD and SR_FLAG_QUADRANT_MAPPED_FORWARD exclude each other");
    if (rows && (!reference || counters || !cull))
        return fail(SR_ERR_UNSUPPORTED, "SR_FLAG_ROW_MAPPED_FORWARD: 16x16 tile, three colour channels, no counters, culling on");
    if ((pair & SR_FLAG_ROW_BACKWARD) && (!reference || counters || !cull || quads || fwd_only))
        return fail(SR_ERR_UNSUPPORTED, "SR_FLAG_ROW_BACKWARD: 16x16 tile, three colour channels, no counters, culling on, the row-mapped forward, a backward to follow");
    out->cull = cull;
    out->mask = HitMaskFormat::kQuadrant;
    out->backward = BackwardBlend::kOneWave;
    out->forward = counters ? ForwardBlend::kCounting : ForwardBlend::kQuadrantBands;
    if (!reference) return SR_OK;
    out->backward = (pair & SR_FLAG_ROW_BACKWARD) ? BackwardBlend::kRows
                    : (pair & SR_FLAG_ONE_WAVE_BACKWARD) ? BackwardBlend::kOneWave
                    : (pair & SR_FLAG_COOP_BACKWARD) ? BackwardBlend::kCoop : BackwardBlend::kByTileCount;
    if (counters) return SR_OK;   // (beats everything else)
    if (cull && !rows && !quads && (pair & SR_FLAG_COOP_BACKWARD)) out->forward = ForwardBlend::kCoop;
    else if (pair & SR_FLAG_ROW_BACKWARD) { out->forward = ForwardBlend::kRowsCellMasks; out->mask = HitMaskFormat::kCell; }
    else if (rows) out->forward = ForwardBlend::kRows;
    else if (cull && !quads) out->forward = ForwardBlend::kDevicePicked;
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_abi_version(void) { return SR_ABI_VERSION; }
uint32_t sr_build_switches(void) { return SR_SWITCH_BITS; }
const char* sr_last_error(void) { return g_err; }

size_t sr_geom_bytes(int32_t P) { return geom_layout(P).total; }
size_t sr_binning_bytes(int32_t P, uint32_t num_rendered, int32_t W, int32_t H) { (void)P; return bin_layout(num_rendered, W, H).total; }
size_t sr_image_bytes(int32_t W, int32_t H) { return img_layout(W, H).total; }
size_t sr_backward_workspace_bytes(int32_t P, uint32_t num_rendered, int32_t color_channels) { (void)P; return workspace_layout(num_rendered, color_channels).total; }

int sr_geom_view(void* geom, size_t geom_bytes, int32_t P, SrGeomView* out) {
    if (!geom || !out) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    const GeomLayout L = geom_layout(P);
    if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
    const GeomView G = geom_view(geom, L);
    out->splats = reinterpret_cast<float*>(G.recs); out->depth_keys = G.depth_keys;
    out->tiles_touched = G.tiles_touched; out->clamped = G.clamped;
    out->sorted_gid = G.sorted_gid;
    out->frame_counts = G.counts;
    return SR_OK;
}

int sr_binning_view(void* binning, size_t binning_bytes, int32_t P, uint32_t D, int32_t W, int32_t H, SrBinningView* out) {
    (void)P;
    if (!binning || !out) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    const BinLayout L = bin_layout(D, W, H);
    if (binning_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "binning buffer %zu < %zu", binning_bytes, L.total);
    const BinView B = bin_view(binning, L);
    out->point_list = B.point_list;
    out->ranges = reinterpret_cast<uint32_t*>(B.ranges); out->tile_order = B.order;
    return SR_OK;
}

int sr_image_view(void* image, size_t image_bytes, int32_t W, int32_t H, SrImageView* out) {
    if (!image || !out) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    const ImgLayout L = img_layout(W, H);
    if (image_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "image buffer %zu < %zu", image_bytes, L.total);
    const ImgView I = img_view(image, L);
    out->final_T = I.final_T; out->n_contrib = I.n_contrib;
    return SR_OK;
}

int sr_forward_plan(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, int32_t* radii,
                    uint32_t* num_rendered_host, void* stream) {
    if (int rc = check_common(frame, g)) return rc;
    if (!num_rendered_host) return fail(SR_ERR_INVALID_ARGUMENT, "num_rendered_host is NULL");
    *num_rendered_host = 0;
    const int P = g->P;
    if (P == 0) return SR_OK;
    if (!geom || !radii) return fail(SR_ERR_INVALID_ARGUMENT, "geom / radii is NULL");
    const GeomLayout L = geom_layout(P);
    if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
    const GeomView G = geom_view(geom, L);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameDev f = make_frame(frame, g);
    f.sh_jac = (frame->flags & SR_FLAG_FORWARD_ONLY) ? nullptr : G.sh_jac;   // (forward only: K8, its one reader, will not run)
    {
        StageTimer t(SR_STAGE_PREPROCESS, s);
        SR_HIP(launch_preprocess_forward(P, f, *g, G.recs, G.depth_keys, G.tiles_touched, G.rect, G.clamped, radii, s));
    }
    if (int rc = debug_sync(frame, s, "preprocess_forward")) return rc;
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(s, (frame->flags & SR_FLAG_BALLOT_RANKING) != 0, &sort_mode)) return rc;   // (first call on a device: ~20 us self-check)
    // D, the scan's grand total, is the one word the host reads back (the reference does the same between scan and duplicateWithKeys).
    // It travels through a pinned host word (one block per host thread; with one event per (thread, device) the only things this library
    // keeps): the last scan kernel stores it there itself when the word is mapped into the device's address space -- no copy kernel
    // between the scan and the host's wake-up -- else a DMA copy does.
    // SR_FLAG_BINNING_CAPACITY, the sync-free forward: D stays on the device (SrGeomView.frame_counts); no pinned word, no event, no host
    // wait -- nothing in this call that a stream capture could not record.
    const bool read_back = !(frame->flags & SR_FLAG_BINNING_CAPACITY);
    uint32_t* pinned = read_back ? pinned_words() : nullptr;
    uint32_t* pinned_dev = nullptr;
    if (pinned && (hipHostGetDevicePointer(reinterpret_cast<void**>(&pinned_dev), pinned, 0) != hipSuccess)) pinned_dev = nullptr;
    {
        StageTimer t(SR_STAGE_SCAN, s);
        SR_HIP(run_tile_count_scan(P, G.tiles_touched, G.first, G.block_base, L.base_bytes, pinned_dev, s));
    }
    if (int rc = debug_sync(frame, s, "emission_scan")) return rc;
    // The depth sort is queued BEHIND the read-back and the host waits for the read-back only, so the GPU sorts while the caller wakes
    // up, sizes the binning buffer from D and queues the second phase.
    hipEvent_t copied = nullptr;
    if (read_back) {
        static thread_local hipEvent_t copied_ev[kMaxDevices] = {};   // one marker per (calling thread, device): an event belongs to its device
        int dev = 0;
        SR_HIP(hipGetDevice(&dev));
        if (dev >= 0 && dev < kMaxDevices) {
            if (!copied_ev[dev] && hipEventCreateWithFlags(&copied_ev[dev], hipEventDisableTiming) != hipSuccess) copied_ev[dev] = nullptr;
            copied = copied_ev[dev];
        }
        if (!pinned_dev) SR_HIP(hipMemcpyAsync(pinned ? pinned : num_rendered_host, G.counts + kCountDuplicates, 4, hipMemcpyDeviceToHost, s));
        if (copied && pinned && hipEventRecord(copied, s) != hipSuccess) copied = nullptr;   // (then: wait for the stream instead)
    }
    {
        StageTimer t(SR_STAGE_DEPTH_SORT, s);
        SR_HIP(run_depth_sort(P, G.depth_keys, G.rect, G.sorted_keys, G.sorted_gid, G.rect_sorted, G.temp, L.temp_bytes, sort_mode,
                              (frame->flags & SR_FLAG_ONE_SWEEP_SORT) != 0, f.tiles_x, f.tiles_y, G.counts + kCountVisible, s));
    }
    if (!read_back) {
        *num_rendered_host = 0xFFFFFFFFu;   // unknown to the host
        return debug_sync(frame, s, "depth_sort");
    }
    if (int rc = debug_sync(frame, s, "depth_sort")) return rc;
    if (copied && pinned) SR_HIP(hipEventSynchronize(copied));
    else SR_HIP(hipStreamSynchronize(s));
    if (pinned) *num_rendered_host = *reinterpret_cast<volatile uint32_t*>(pinned);
    return SR_OK;
}

namespace {
// K3..K5 (duplicate emission, tile partition, tile ranges + dispatch order): shared by the blend forward and the per-class pass
int bin_duplicates(const SrFrame* frame, const SrGaussians* g, const FrameDev& f, void* geom, size_t geom_bytes, const BinView& B,
                   uint32_t D, hipStream_t s, float4** recs_out) {
    const int P = g->P;
    const int n_tiles = f.tiles_x * f.tiles_y;
    *recs_out = nullptr;
    if (P > 0 && D > 0) {
        if (!geom) return fail(SR_ERR_INVALID_ARGUMENT, "geom is NULL");
        const GeomLayout L = geom_layout(P);
        if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
        const GeomView G = geom_view(geom, L);
        *recs_out = G.recs;
        if (f.tiles_x > kMaxTilesPerAxis || f.tiles_y > kMaxTilesPerAxis)
            return fail(SR_ERR_INVALID_ARGUMENT, "%d x %d tiles: at most %d per axis (use a larger tile)", f.tiles_x, f.tiles_y, kMaxTilesPerAxis);
        if (L.temp_bytes < expand_x_hist_bytes(P, f.tiles_x)) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom scratch too small for the column histogram");
        RankMode sort_mode = kRankUnknown;
        if (int rc = rank_mode(s, (frame->flags & SR_FLAG_BALLOT_RANKING) != 0, &sort_mode)) return rc;
        if (frame->flags & SR_FLAG_BINNING_CAPACITY)   // D = the caller's capacity: does the frame fit?  (else: nothing is binned, the flag is set)
            SR_HIP(run_capacity_guard(G.counts, D, s));
        {
            StageTimer t(SR_STAGE_EXPAND_X, s);
            SR_HIP(run_expand_columns(P, f.tiles_x, n_tiles, G.rect_sorted, G.sorted_gid, B.columns, B.n_columns, static_cast<uint32_t*>(G.temp), B.row_total,
                                      B.tile_counts, sort_mode, G.counts + kCountVisible, s));
        }
        if (int rc = debug_sync(frame, s, "expand_columns")) return rc;
        {
            StageTimer t(SR_STAGE_EXPAND_Y, s);
            SR_HIP(run_expand_rows(D, f.tiles_x, f.tiles_y, B.columns, B.n_columns, B.hist, B.row_total, B.point_list, B.tile_counts, sort_mode, s));
        }
        if (int rc = debug_sync(frame, s, "expand_rows")) return rc;
    } else {
        SR_HIP(launch_zero_bytes(B.tile_counts, sizeof(uint32_t) * (size_t)n_tiles, s));   // (no partition ran)
    }
    {
        StageTimer t(SR_STAGE_RANGES, s);
        SR_HIP(run_tile_ranges_order(n_tiles, B.tile_counts, B.ranges, B.order, s));
    }
    return debug_sync(frame, s, "tile_ranges");
}

// per-class state between the forward and the backward of the class pass.  (The class-ordered copy of the tile lists lives in the binning
// buffer's `columns` region -- the column items of the expanding partition are dead once pass Y has run -- and the class id bytes in the
// geometry buffer's `sh_jac` region: the class pass has no SH colour.)
struct ClassLayout { size_t state, last, tile_total, ranges, total; };
ClassLayout class_layout(int W, int H, int n_classes) {
    ClassLayout L{};
    const size_t hw = (size_t)(W > 0 ? W : 1) * (size_t)(H > 0 ? H : 1), n = (size_t)(n_classes > 0 ? n_classes : 1);
    const size_t tiles = (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8);   // (sized for the smallest tile of the sweep, 8x8)
    Carver c;
    L.state = c.take(n * 3 * hw * 4);
    L.last = c.take(n * hw * 4);
    L.tile_total = c.take((tiles > 0 ? tiles : 1) * n * 4);
    L.ranges = c.take((tiles > 0 ? tiles : 1) * n * 8);
    L.total = c.off;
    return L;
}
struct ClassView { float* state; uint32_t* last; uint32_t* tile_total; uint2* ranges; };
ClassView class_view(void* class_image, const ClassLayout& L) {
    return ClassView{at<float>(class_image, L.state), at<uint32_t>(class_image, L.last), at<uint32_t>(class_image, L.tile_total), at<uint2>(class_image, L.ranges)};
}

// The preconditions of the four class entry points.  They differ in where the class ids come from -- column 0 of colors_precomp[P,3] (the
// stand-alone pass) or an int32 array of their own (the pass on the binning of a colour pass, whose colours stay what they are) -- and in
// whether a precomputed transMat is refused.
enum class ClassIds { kInColors, kOwnArray };
int check_class_pass(const SrFrame* frame, const SrGaussians* g, int n_classes, ClassIds ids, bool refuse_transmat) {
    if (int rc = check_common(frame, g)) return rc;
    if (frame->flags & SR_FLAG_BINNING_CAPACITY) return fail(SR_ERR_UNSUPPORTED, "SR_FLAG_BINNING_CAPACITY serves the operator (sr_forward_* / sr_backward*), not the per-class pass");
    if (n_classes < 1 || n_classes > 6) return fail(SR_ERR_UNSUPPORTED, "n_classes %d not in 1..6", n_classes);
    // (every tile shape check_common accepts: 8x8, 16x8, 16x16, 32x8, 32x16)
    if (ids == ClassIds::kInColors && g->P > 0 && (g->shs || !g->colors_precomp || (g->color_channels != 0 && g->color_channels != 3)))
        return fail(SR_ERR_INVALID_ARGUMENT, "the per-class distortion pass takes the class ids in colors_precomp[P,3] (column 0), no SHs");
    if (refuse_transmat && g->transMat_precomp) return fail(SR_ERR_UNSUPPORTED, "the per-class pass takes scales and rotations, not a precomputed transMat");
    return SR_OK;
}
}  // namespace

int sr_forward_render(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning,
                      size_t binning_bytes, void* image, size_t image_bytes, uint32_t D, float* out_color,
                      float* out_allmap, void* stream) {
    if (int rc = check_common(frame, g)) return rc;
    const FrameDev f = make_frame(frame, g);
    BlendChoice blend;
    if (int rc = choose_blend(frame, f, true, &blend)) return rc;
    const bool fwd_only = (frame->flags & SR_FLAG_FORWARD_ONLY) != 0;   // no backward follows: its state (image buffer, hit masks) is not written
    if (!binning || (!image && !fwd_only) || !out_color || !out_allmap) return fail(SR_ERR_INVALID_ARGUMENT, "binning / image / out_color / out_allmap is NULL");
    const int W = frame->image_width, H = frame->image_height;
    const BinLayout BL = bin_layout(D, W, H);
    const ImgLayout IL = img_layout(W, H);
    if (binning_bytes < BL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "binning buffer %zu < %zu", binning_bytes, BL.total);
    if (!fwd_only && image_bytes < IL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "image buffer %zu < %zu", image_bytes, IL.total);
    const BinView B = bin_view(binning, BL);
    const ImgView I = fwd_only ? ImgView{nullptr, nullptr} : img_view(image, IL);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float4* recs = nullptr;
    if (int rc = bin_duplicates(frame, g, f, geom, geom_bytes, B, D, s, &recs)) return rc;
    {
        StageTimer t(SR_STAGE_BLEND_FWD, s);
        const GeomView G = geom_view(geom, geom_layout(g->P));   // (D and the visible count, left in the geometry state by the emission scan)
        SR_HIP(launch_render_forward(f, B.ranges, B.order, B.point_list, recs, g->colors_precomp, out_color, out_allmap, I.final_T, I.n_contrib,
                                     fwd_only ? nullptr : B.hit_mask, blend, reinterpret_cast<unsigned long long*>(frame->blend_counters), G.counts, s));
    }
    return debug_sync(frame, s, "render_forward");
}

size_t sr_class_image_bytes(int32_t W, int32_t H, int32_t n_classes) { return class_layout(W, H, n_classes).total; }

int sr_class_forward_render(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                            size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t D, float* out_dist, void* stream) {
    if (int rc = check_class_pass(frame, g, n_classes, ClassIds::kInColors, false)) return rc;
    if (!binning || !class_image || !out_dist) return fail(SR_ERR_INVALID_ARGUMENT, "binning / class_image / out_dist is NULL");
    if (g->P > 0 && !geom) return fail(SR_ERR_INVALID_ARGUMENT, "geom is NULL (the class ids of the P Gaussians are staged in it, even when no duplicate was emitted)");
    const int W = frame->image_width, H = frame->image_height;
    const BinLayout BL = bin_layout(D, W, H);
    const ClassLayout CL = class_layout(W, H, n_classes);
    if (binning_bytes < BL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "binning buffer %zu < %zu", binning_bytes, BL.total);
    if (class_image_bytes < CL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "class image buffer %zu < %zu", class_image_bytes, CL.total);
    const BinView B = bin_view(binning, BL);
    const ClassView C = class_view(class_image, CL);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameDev f = make_frame(frame, g);
    float4* recs = nullptr;
    if (int rc = bin_duplicates(frame, g, f, geom, geom_bytes, B, D, s, &recs)) return rc;
    {
        // every tile list, stably partitioned by class: [class 0 by depth | class 1 by depth | ...] + a (begin, end) pair per (tile, class)
        StageTimer t(SR_STAGE_CLASS_PARTITION, s);
        uint8_t* ids = g->P > 0 && geom ? reinterpret_cast<uint8_t*>(geom_view(geom, geom_layout(g->P)).sh_jac) : nullptr;
        SR_HIP(launch_class_partition(g->P, f.tiles_x * f.tiles_y, n_classes, g->colors_precomp, nullptr, B.ranges, B.point_list, ids, B.class_list(), C.ranges, s));
    }
    if (int rc = debug_sync(frame, s, "class_partition")) return rc;
    {
        StageTimer t(SR_STAGE_CLASS_FWD, s);
        SR_HIP(launch_class_forward(f, n_classes, C.ranges, B.order, B.class_list(), recs, out_dist, C.state, C.last, C.tile_total, B.hit_mask,
                                    (frame->flags & SR_FLAG_NO_QUADRANT_CULL) ? 0 : 1, s));
    }
    return debug_sync(frame, s, "class_forward");
}

int sr_class_backward(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* radii, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t D, const float* dL_ddist,
                      void* workspace, size_t workspace_bytes, const SrGradients* grads, void* stream) {
    if (int rc = check_class_pass(frame, g, n_classes, ClassIds::kInColors, false)) return rc;
    if (int rc = check_backward_frame(frame)) return rc;
    if (!grads) return fail(SR_ERR_INVALID_ARGUMENT, "grads is NULL");
    const int P = g->P;
    if (P == 0) return SR_OK;
    if (!radii || !geom || !binning || !class_image || !dL_ddist || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL buffer argument");
    const int W = frame->image_width, H = frame->image_height;
    const GeomLayout L = geom_layout(P);
    const BinLayout BL = bin_layout(D, W, H);
    const ClassLayout CL = class_layout(W, H, n_classes);
    if (geom_bytes < L.total || binning_bytes < BL.total || class_image_bytes < CL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "state buffer too small");
    if (workspace_bytes < workspace_layout(D, 3).total) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, workspace_layout(D, 3).total);
    const GeomView G = geom_view(geom, L);
    const BinView B = bin_view(binning, BL);
    const ClassView C = class_view(class_image, CL);
    const WorkspaceView ws = workspace_view(workspace, D, 3);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameDev f = make_frame(frame, g);
    f.first = G.first; f.first_base = G.block_base; f.sh_jac = G.sh_jac;
    {
        StageTimer t(SR_STAGE_CLASS_BWD, s);
        if (D > 0) SR_HIP(launch_zero_bytes(ws.written, D, s));
        if (D > 0)
            SR_HIP(launch_class_backward(f, n_classes, C.ranges, B.order, B.class_list(), G.recs, C.state, C.last, C.tile_total, dL_ddist, B.hit_mask,
                                         ws.records, ws.written, 0, s));
    }
    if (int rc = debug_sync(frame, s, "class_backward")) return rc;
    {
        StageTimer t(SR_STAGE_PREPROCESS_BWD, s);
        SR_HIP(launch_preprocess_backward(P, f, *g, radii, G.clamped, G.recs, ws.records, ws.written, G.tiles_touched, *grads, s));
    }
    return debug_sync(frame, s, "preprocess_backward");
}

// ---- the per-class pass on the binning of a colour pass (one plan, one binning, one K8 for both: SURVEY.md 8f N1 in full) -------------
namespace {
struct ClassSharedLayout { ClassLayout C; size_t ids, hit, total; };
ClassSharedLayout class_shared_layout(int P, int W, int H, int n_classes, uint32_t D) {
    ClassSharedLayout L{};
    L.C = class_layout(W, H, n_classes);
    Carver c{L.C.total};                           // behind the stand-alone pass's regions
    L.ids = c.take((size_t)(P > 0 ? P : 1));       // class byte per Gaussian (the colour pass owns the sh_jac region here)
    L.hit = c.take((size_t)(D > 0 ? D : 1) * 2);   // this pass's own (entry, quadrant) hit masks: the colour pass keeps the binning buffer's
    L.total = c.off;
    return L;
}
}  // namespace

size_t sr_class_shared_bytes(int32_t P, int32_t W, int32_t H, int32_t n_classes, uint32_t D) { return class_shared_layout(P, W, H, n_classes, D).total; }

int sr_class_forward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* classes, void* geom, size_t geom_bytes,
                            void* binning, size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t D, float* out_dist, void* stream) {
    if (int rc = check_class_pass(frame, g, n_classes, ClassIds::kOwnArray, true)) return rc;
    if (!binning || !class_state || !out_dist || (g->P > 0 && !classes)) return fail(SR_ERR_INVALID_ARGUMENT, "binning / class_state / out_dist / classes is NULL");
    const int W = frame->image_width, H = frame->image_height, P = g->P;
    const BinLayout BL = bin_layout(D, W, H);
    const ClassSharedLayout SL = class_shared_layout(P, W, H, n_classes, D);
    if (binning_bytes < BL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "binning buffer %zu < %zu", binning_bytes, BL.total);
    if (class_state_bytes < SL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "class state buffer %zu < %zu", class_state_bytes, SL.total);
    float4* recs = nullptr;
    if (P > 0 && D > 0) {
        if (!geom) return fail(SR_ERR_INVALID_ARGUMENT, "geom is NULL");
        const GeomLayout L = geom_layout(P);
        if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
        recs = geom_view(geom, L).recs;
    }
    const BinView B = bin_view(binning, BL);
    const ClassView C = class_view(class_state, SL.C);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameDev f = make_frame(frame, g);
    {
        StageTimer t(SR_STAGE_CLASS_PARTITION, s);
        SR_HIP(launch_class_partition(P, f.tiles_x * f.tiles_y, n_classes, nullptr, classes, B.ranges, B.point_list, at<uint8_t>(class_state, SL.ids), B.class_list(),
                                      C.ranges, s));
    }
    if (int rc = debug_sync(frame, s, "class_partition")) return rc;
    {
        StageTimer t(SR_STAGE_CLASS_FWD, s);
        SR_HIP(launch_class_forward(f, n_classes, C.ranges, B.order, B.class_list(), recs, out_dist, C.state, C.last, C.tile_total, at<uint16_t>(class_state, SL.hit),
                                    (frame->flags & SR_FLAG_NO_QUADRANT_CULL) ? 0 : 1, s));
    }
    return debug_sync(frame, s, "class_forward");
}

int sr_class_backward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                             size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t D, const float* dL_ddist, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (int rc = check_class_pass(frame, g, n_classes, ClassIds::kOwnArray, false)) return rc;
    if (int rc = check_backward_frame(frame)) return rc;
    const int P = g->P;
    if (P == 0 || D == 0) return SR_OK;
    if (!geom || !binning || !class_state || !dL_ddist || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL buffer argument");
    const int W = frame->image_width, H = frame->image_height;
    const GeomLayout L = geom_layout(P);
    const BinLayout BL = bin_layout(D, W, H);
    const ClassSharedLayout SL = class_shared_layout(P, W, H, n_classes, D);
    if (geom_bytes < L.total || binning_bytes < BL.total || class_state_bytes < SL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "state buffer too small");
    const size_t ws_bytes = workspace_layout(D, g->color_channels).total;
    if (workspace_bytes < ws_bytes) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, ws_bytes);
    const GeomView G = geom_view(geom, L);
    const BinView B = bin_view(binning, BL);
    const ClassView C = class_view(class_state, SL.C);
    // the records and flags sr_backward_blend of the SAME frame left in the workspace: this pass adds to them
    const WorkspaceView ws = workspace_view(workspace, D, g->color_channels);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameDev f = make_frame(frame, g);
    f.first = G.first; f.first_base = G.block_base;
    {
        StageTimer t(SR_STAGE_CLASS_BWD, s);
        SR_HIP(launch_class_backward(f, n_classes, C.ranges, B.order, B.class_list(), G.recs, C.state, C.last, C.tile_total, dL_ddist, at<uint16_t>(class_state, SL.hit),
                                     ws.records, ws.written, (int)(record_bytes(g->color_channels) / 16), s));
    }
    return debug_sync(frame, s, "class_backward_shared");
}

namespace {
struct BackwardCtx {
    int P; GeomView G; BinView B; ImgView I; WorkspaceView ws; FrameDev f; BlendChoice blend; hipStream_t s;
};
// argument checks and buffer carving shared by the backward entry points
int backward_ctx(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                 void* image, size_t image_bytes, uint32_t D, void* workspace, size_t workspace_bytes, void* stream, BackwardCtx* c) {
    if (int rc = check_common(frame, g)) return rc;
    if (int rc = check_backward_frame(frame)) return rc;
    c->f = make_frame(frame, g);
    if (int rc = choose_blend(frame, c->f, false, &c->blend)) return rc;
    c->P = g->P;
    if (c->P == 0) return SR_OK;
    if (!geom || !binning || !image || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL buffer argument");
    const int W = frame->image_width, H = frame->image_height;
    const GeomLayout L = geom_layout(c->P);
    const BinLayout BL = bin_layout(D, W, H);
    const ImgLayout IL = img_layout(W, H);
    if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
    if (binning_bytes < BL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "binning buffer %zu < %zu", binning_bytes, BL.total);
    if (image_bytes < IL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "image buffer %zu < %zu", image_bytes, IL.total);
    const size_t ws_bytes = workspace_layout(D, g->color_channels).total;
    if (workspace_bytes < ws_bytes) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, ws_bytes);
    c->G = geom_view(geom, L); c->B = bin_view(binning, BL); c->I = img_view(image, IL);
    c->ws = workspace_view(workspace, D, g->color_channels);
    c->s = static_cast<hipStream_t>(stream);
    set_backward_state(&c->f, frame, c->G);
    return SR_OK;
}
}  // namespace

int sr_backward_blend(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                      void* image, size_t image_bytes, uint32_t D, const float* dL_dcolor, const float* dL_dallmap, void* workspace,
                      size_t workspace_bytes, void* stream) {
    BackwardCtx c;
    if (int rc = backward_ctx(frame, g, geom, geom_bytes, binning, binning_bytes, image, image_bytes, D, workspace, workspace_bytes, stream, &c)) return rc;
    if (c.P == 0) return SR_OK;
    if (!dL_dcolor || !dL_dallmap) return fail(SR_ERR_INVALID_ARGUMENT, "dL_dcolor / dL_dallmap is NULL");
    {
        StageTimer t(SR_STAGE_BLEND_BWD, c.s);
        if (D > 0) SR_HIP(launch_zero_bytes(c.ws.written, D, c.s));
        if (D > 0)
            SR_HIP(launch_render_backward(c.f, c.B.ranges, c.B.order, c.B.point_list, c.G.recs, g->colors_precomp, c.I.final_T, c.I.n_contrib, dL_dcolor, dL_dallmap,
                                          c.B.hit_mask, c.ws.records, c.ws.written, !(frame->flags & SR_FLAG_NO_PRECOMP_COLOR_GRAD), c.blend.backward, c.s));
    }
    return debug_sync(frame, c.s, "render_backward");
}

int sr_backward_colors(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes, uint32_t D,
                       void* workspace, size_t workspace_bytes, float* dL_dcolors, void* stream) {
    if (int rc = check_common(frame, g)) return rc;
    if (int rc = check_backward_frame(frame)) return rc;
    const int P = g->P;
    if (P == 0) return SR_OK;
    if (g->color_channels == 6 || g->color_channels == 9) return fail(SR_ERR_UNSUPPORTED, "sr_backward_colors serves the 3-channel pass");
    if (!radii || !geom || !workspace || !dL_dcolors) return fail(SR_ERR_INVALID_ARGUMENT, "NULL buffer argument");
    const GeomLayout L = geom_layout(P);
    if (geom_bytes < L.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "geom buffer %zu < %zu", geom_bytes, L.total);
    if (workspace_bytes < workspace_layout(D, g->color_channels).total) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace too small");
    const GeomView G = geom_view(geom, L);
    const WorkspaceView ws = workspace_view(workspace, D, g->color_channels);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameDev f = make_frame(frame, g);
    set_backward_state(&f, frame, G);
    StageTimer t(SR_STAGE_PREPROCESS_BWD, s);
    SR_HIP(launch_color_gradients(P, f, radii, G.clamped, G.recs, ws.records, ws.written, G.tiles_touched, g->shs != nullptr, dL_dcolors, s));
    return debug_sync(frame, s, "color_gradients");
}

int sr_backward_geometry(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                         void* binning, size_t binning_bytes, void* image, size_t image_bytes, uint32_t D, void* workspace,
                         size_t workspace_bytes, const SrGradients* grads, void* stream) {
    if (!grads) return fail(SR_ERR_INVALID_ARGUMENT, "grads is NULL");
    BackwardCtx c;
    if (int rc = backward_ctx(frame, g, geom, geom_bytes, binning, binning_bytes, image, image_bytes, D, workspace, workspace_bytes, stream, &c)) return rc;
    if (c.P == 0) return SR_OK;
    if (!radii) return fail(SR_ERR_INVALID_ARGUMENT, "radii is NULL");
    {
        StageTimer t(SR_STAGE_PREPROCESS_BWD, c.s);
        SR_HIP(launch_preprocess_backward(c.P, c.f, *g, radii, c.G.clamped, c.G.recs, c.ws.records, c.ws.written, c.G.tiles_touched, *grads, c.s));
    }
    return debug_sync(frame, c.s, "preprocess_backward");
}

int sr_backward(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                void* binning, size_t binning_bytes, void* image, size_t image_bytes, uint32_t D, const float* dL_dcolor,
                const float* dL_dallmap, void* workspace, size_t workspace_bytes, const SrGradients* grads, void* stream) {
    if (!grads) return fail(SR_ERR_INVALID_ARGUMENT, "grads is NULL");
    if (int rc = sr_backward_blend(frame, g, geom, geom_bytes, binning, binning_bytes, image, image_bytes, D, dL_dcolor, dL_dallmap, workspace, workspace_bytes, stream)) return rc;
    return sr_backward_geometry(frame, g, radii, geom, geom_bytes, binning, binning_bytes, image, image_bytes, D, workspace, workspace_bytes, grads, stream);
}

int sr_debug_pair_decisions(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                            uint32_t D, uint64_t* valid_bits, uint64_t* use3d_bits, void* stream) {
    if (int rc = check_common(frame, g)) return rc;
    if (g->P == 0 || D == 0) return SR_OK;
    if (!geom || !binning || !valid_bits || !use3d_bits) return fail(SR_ERR_INVALID_ARGUMENT, "NULL buffer argument");
    const GeomLayout L = geom_layout(g->P);
    const BinLayout BL = bin_layout(D, frame->image_width, frame->image_height);
    if (geom_bytes < L.total || binning_bytes < BL.total) return fail(SR_ERR_BUFFER_TOO_SMALL, "state buffer too small");
    const BinView B = bin_view(binning, BL);
    const FrameDev f = make_frame(frame, g);
    SR_HIP(launch_pair_decisions(f, B.ranges, B.point_list, geom_view(geom, L).recs,
                                 reinterpret_cast<unsigned long long*>(valid_bits), reinterpret_cast<unsigned long long*>(use3d_bits), static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_sh_gradient_expand(int32_t P, int32_t sh_coeffs, int32_t sh_degree, int32_t n_views, const float* means3D,
                          const float* campos, const float* dL_dcolors, float* dL_dsh, void* stream) {
    if (P < 0 || n_views < 1) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0 or n_views < 1");
    if (sh_degree < 0 || sh_degree > 3) return fail(SR_ERR_UNSUPPORTED, "sh_degree %d not in 0..3", sh_degree);
    if (sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) return fail(SR_ERR_INVALID_ARGUMENT, "shs has %d coefficients, degree %d needs %d", sh_coeffs, sh_degree, (sh_degree + 1) * (sh_degree + 1));
    if (P == 0) return SR_OK;
    if (!means3D || !campos || !dL_dcolors || !dL_dsh) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    SR_HIP(launch_sh_gradient_expand(P, sh_coeffs, sh_degree, n_views, means3D, campos, dL_dcolors, dL_dsh, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

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
    if (workspace_bytes < knn_workspace_bytes(nq, n_reference)) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, knn_workspace_bytes(nq, n_reference));
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), false, &sort_mode)) return rc;
    SR_HIP(knn_mean_dist2(nq, query, n_reference, reference, K, take_sqrt, out, workspace, workspace_bytes, sort_mode, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

size_t sr_cluster_workspace_bytes(int32_t n) { return cluster_workspace_bytes(n > 0 ? n : 0); }

int sr_cluster_radius(int32_t n, const float* xyz, const uint8_t* active, float radius, int64_t* labels, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "negative point count");
    if (!(radius >= 0.f && radius <= FLT_MAX)) return fail(SR_ERR_INVALID_ARGUMENT, "radius %g is not a finite number >= 0", (double)radius);
    if (n == 0) return SR_OK;
    if (!xyz || !labels || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (workspace_bytes < cluster_workspace_bytes(n)) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, cluster_workspace_bytes(n));
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), false, &sort_mode)) return rc;
    SR_HIP(cluster_radius(n, xyz, active, radius, labels, workspace, workspace_bytes, sort_mode, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream) {
    (void)projmatrix;
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P == 0) return SR_OK;
    if (!means3D || !viewmatrix || !present) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    SR_HIP(launch_mark_visible(P, means3D, viewmatrix, present, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

static int post_cam(int32_t W, int32_t H, float fovx, float fovy, float depth_ratio, const float* viewmatrix, PostCam* cam) {
    if (W <= 0 || H <= 0 || !viewmatrix) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size / NULL viewmatrix");
    cam->W = W; cam->H = H;
    cam->fx = (float)W / (2.f * tanf(fovx * 0.5f)); cam->fy = (float)H / (2.f * tanf(fovy * 0.5f));
    cam->depth_ratio = depth_ratio; cam->view = viewmatrix;
    return SR_OK;
}

int sr_postprocess_forward(int32_t W, int32_t H, float fovx, float fovy, float depth_ratio, const float* viewmatrix,
                           const float* allmap, float* rend_normal, float* surf_depth, float* surf_normal, float* surf_point,
                           void* stream) {
    PostCam cam;
    if (int rc = post_cam(W, H, fovx, fovy, depth_ratio, viewmatrix, &cam)) return rc;
    if (!allmap || !rend_normal || !surf_depth || !surf_normal || !surf_point) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    SR_HIP(launch_postprocess_forward(cam, allmap, rend_normal, surf_depth, surf_normal, surf_point, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_postprocess_backward(int32_t W, int32_t H, float fovx, float fovy, float depth_ratio, const float* viewmatrix,
                            const float* allmap, const float* g_rend_normal, const float* g_surf_depth, const float* g_surf_normal,
                            const float* g_surf_point, float* scratch6, float* g_allmap, void* stream) {
    PostCam cam;
    if (int rc = post_cam(W, H, fovx, fovy, depth_ratio, viewmatrix, &cam)) return rc;
    if (!allmap || !scratch6 || !g_allmap) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    SR_HIP(launch_postprocess_backward(cam, allmap, g_rend_normal, g_surf_depth, g_surf_normal, g_surf_point, scratch6, g_allmap,
                                       static_cast<hipStream_t>(stream)));
    return SR_OK;
}

size_t sr_image_loss_workspace_bytes(int32_t W, int32_t H, int32_t C) {
    if (W <= 0 || H <= 0 || C <= 0) return 0;
    return image_loss_partial_bytes() + 3 * sizeof(float) * (size_t)W * (size_t)H * (size_t)C;
}

static int image_loss_args(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                           const float* alpha, const void* workspace, size_t workspace_bytes, LossImages* a) {
    if (W <= 0 || H <= 0 || C <= 0) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d with %d channels", W, H, C);
    if (!image || !gt || !workspace) return fail(SR_ERR_INVALID_ARGUMENT, "image / gt / workspace is NULL");
    if ((sky != nullptr) != (alpha != nullptr)) return fail(SR_ERR_INVALID_ARGUMENT, "sky and alpha go together: give both or neither");
    if (!image_loss_supported(W, H, C)) return fail(SR_ERR_UNSUPPORTED, "%dx%d with %d channels is beyond the launch limits", W, H, C);
    if (workspace_bytes < sr_image_loss_workspace_bytes(W, H, C))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, sr_image_loss_workspace_bytes(W, H, C));
    *a = LossImages{W, H, C, lambda_dssim, image, gt, sky, alpha};
    return SR_OK;
}

int sr_image_loss_forward(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                          const float* alpha, void* workspace, size_t workspace_bytes, float* out3, void* stream) {
    LossImages a;
    if (int rc = image_loss_args(W, H, C, lambda_dssim, image, gt, sky, alpha, workspace, workspace_bytes, &a)) return rc;
    if (!out3) return fail(SR_ERR_INVALID_ARGUMENT, "out3 is NULL");
    SR_HIP(launch_image_loss_forward(a, workspace, out3, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_image_loss_backward(int32_t W, int32_t H, int32_t C, float lambda_dssim, const float* image, const float* gt, const float* sky,
                           const float* alpha, const void* workspace, size_t workspace_bytes, const float* g_loss, float* g_image,
                           float* g_sky, float* g_alpha, void* stream) {
    LossImages a;
    if (int rc = image_loss_args(W, H, C, lambda_dssim, image, gt, sky, alpha, workspace, workspace_bytes, &a)) return rc;
    if (!g_loss || !g_image) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_image is NULL");
    if (sky && (!g_sky || !g_alpha)) return fail(SR_ERR_INVALID_ARGUMENT, "with sky and alpha, g_sky and g_alpha are required");
    SR_HIP(launch_image_loss_backward(a, workspace, g_loss, g_image, g_sky, g_alpha, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

size_t sr_aux_loss_workspace_bytes(int64_t n) { return n > 0 ? aux_loss_workspace_bytes((size_t)n) : 0; }

namespace {

// shared refusals of the auxiliary losses: the element count, then (forwards only: workspace_bytes != nullptr) the workspace
int aux_count(const char* what, int64_t n, const void* workspace, const size_t* workspace_bytes) {
    if (!aux_loss_supported((size_t)n)) return fail(SR_ERR_UNSUPPORTED, "%s: %lld elements are beyond the launch limits", what, (long long)n);
    if (!workspace_bytes) return SR_OK;
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "%s: workspace is NULL", what);
    if (*workspace_bytes < aux_loss_workspace_bytes((size_t)n))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "%s: workspace %zu < %zu", what, *workspace_bytes, aux_loss_workspace_bytes((size_t)n));
    return SR_OK;
}

int semantic_ce_args(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                     CeArgs* a, CeTarget* form) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (C < 1 || C > SR_CE_MAX_CLASSES) return fail(SR_ERR_INVALID_ARGUMENT, "%d classes: not in 1..%d", C, SR_CE_MAX_CLASSES);
    if (label_bytes != 0 && label_bytes != 1 && label_bytes != 4 && label_bytes != 8)
        return fail(SR_ERR_INVALID_ARGUMENT, "label_bytes %d: not 0 (probabilities), 1, 4 or 8", label_bytes);
    if (!logits || !target) return fail(SR_ERR_INVALID_ARGUMENT, "logits / target is NULL");
    static_assert(SR_CE_MAX_CLASSES == kCeMaxClasses, "the header's class limit is the kernels'");
    *form = static_cast<CeTarget>(label_bytes);
    a->C = C;
    a->N = (size_t)W * (size_t)H;
    for (int c = 0; c < kCeMaxClasses; ++c) a->w[c] = c < C ? (weight ? weight[c] : 1.f) : 0.f;
    a->x = logits;
    a->target = target;
    return SR_OK;
}

}  // namespace

int sr_semantic_ce_forward(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                           void* workspace, size_t workspace_bytes, float* out1, void* stream) {
    CeArgs a;
    CeTarget form;
    if (int rc = semantic_ce_args(W, H, C, logits, target, label_bytes, weight, &a, &form)) return rc;
    if (!out1) return fail(SR_ERR_INVALID_ARGUMENT, "out1 is NULL");
    if (int rc = aux_count("sr_semantic_ce_forward", (int64_t)a.N, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_semantic_ce_forward(a, form, workspace, out1, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_semantic_ce_backward(int32_t W, int32_t H, int32_t C, const float* logits, const void* target, int32_t label_bytes, const float* weight,
                            const float* g_loss, float* g_logits, void* stream) {
    CeArgs a;
    CeTarget form;
    if (int rc = semantic_ce_args(W, H, C, logits, target, label_bytes, weight, &a, &form)) return rc;
    if (!g_loss || !g_logits) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_logits is NULL");
    if (int rc = aux_count("sr_semantic_ce_backward", (int64_t)a.N, nullptr, nullptr)) return rc;
    SR_HIP(launch_semantic_ce_backward(a, form, g_loss, g_logits, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_surface_reg_forward(int32_t W, int32_t H, const float* rend_normal, const float* surf_normal, const float* rend_dist, double lambda_normal,
                           double lambda_dist, void* workspace, size_t workspace_bytes, float* out3, void* stream) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (!rend_normal || !surf_normal || !rend_dist || !out3) return fail(SR_ERR_INVALID_ARGUMENT, "rend_normal / surf_normal / rend_dist / out3 is NULL");
    const SurfaceRegArgs a{(size_t)W * (size_t)H, lambda_normal, lambda_dist, rend_normal, surf_normal, rend_dist};
    if (int rc = aux_count("sr_surface_reg_forward", (int64_t)a.N, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_surface_reg_forward(a, workspace, out3, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_surface_reg_backward(int32_t W, int32_t H, const float* rend_normal, const float* surf_normal, double lambda_normal, double lambda_dist,
                            const float* g_loss, float* g_rend_normal, float* g_surf_normal, float* g_rend_dist, void* stream) {
    if (W < 1 || H < 1) return fail(SR_ERR_INVALID_ARGUMENT, "bad image size %dx%d", W, H);
    if (!g_loss) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss is NULL");
    if (g_rend_normal && !surf_normal) return fail(SR_ERR_INVALID_ARGUMENT, "g_rend_normal is asked for without surf_normal");
    if (g_surf_normal && !rend_normal) return fail(SR_ERR_INVALID_ARGUMENT, "g_surf_normal is asked for without rend_normal");
    const SurfaceRegArgs a{(size_t)W * (size_t)H, lambda_normal, lambda_dist, rend_normal, surf_normal, nullptr};
    if (int rc = aux_count("sr_surface_reg_backward", (int64_t)a.N, nullptr, nullptr)) return rc;
    if (!g_rend_normal && !g_surf_normal && !g_rend_dist) return SR_OK;
    SR_HIP(launch_surface_reg_backward(a, g_loss, g_rend_normal, g_surf_normal, g_rend_dist, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_opacity_shrink_forward(int64_t P, const float* opacity, int32_t activated, void* workspace, size_t workspace_bytes, float* out1, void* stream) {
    if (P < 1) return fail(SR_ERR_INVALID_ARGUMENT, "P %lld < 1", (long long)P);
    if (!opacity || !out1) return fail(SR_ERR_INVALID_ARGUMENT, "opacity / out1 is NULL");
    if (int rc = aux_count("sr_opacity_shrink_forward", P, workspace, &workspace_bytes)) return rc;
    SR_HIP(launch_opacity_shrink_forward((size_t)P, opacity, activated != 0, workspace, out1, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_opacity_shrink_backward(int64_t P, const float* opacity, int32_t activated, const float* g_loss, float* g_opacity, void* stream) {
    if (P < 1) return fail(SR_ERR_INVALID_ARGUMENT, "P %lld < 1", (long long)P);
    if (!g_loss || !g_opacity) return fail(SR_ERR_INVALID_ARGUMENT, "g_loss / g_opacity is NULL");
    if (!activated && !opacity) return fail(SR_ERR_INVALID_ARGUMENT, "opacity is NULL");
    if (int rc = aux_count("sr_opacity_shrink_backward", P, nullptr, nullptr)) return rc;
    SR_HIP(launch_opacity_shrink_backward((size_t)P, opacity, activated != 0, g_loss, g_opacity, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

size_t sr_sky_workspace_bytes(int32_t max_workgroups) { return max_workgroups >= 0 ? sky_workspace_bytes(max_workgroups) : 0; }

namespace {

constexpr int kSkyMaxGroups = 1 << 16;

int sky_args(const char* what, int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1,
             const float* w2, const float* b2, const float* w3, const float* b3, int32_t max_workgroups, SkyWeights* p) {
    if (W < 0 || H < 0) return fail(SR_ERR_INVALID_ARGUMENT, "%s: bad image size %dx%d", what, W, H);
    if (max_workgroups < 0 || max_workgroups > kSkyMaxGroups)
        return fail(SR_ERR_INVALID_ARGUMENT, "%s: max_workgroups %d not in 0..%d", what, max_workgroups, kSkyMaxGroups);
    if ((int64_t)W * (int64_t)H > 0x7fffffffll) return fail(SR_ERR_UNSUPPORTED, "%s: %dx%d is 2^31 pixels or more", what, W, H);
    if (!cam || !w0sh || !c || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return fail(SR_ERR_INVALID_ARGUMENT, "%s: cam or a weight pointer is NULL", what);
    *p = SkyWeights{w0sh, c, w1, b1, w2, b2, w3, b3};
    return SR_OK;
}

}  // namespace

int sr_sky_forward(int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, int32_t max_workgroups, float* out, void* stream) {
    SkyWeights p;
    if (int rc = sky_args("sr_sky_forward", W, H, cam, w0sh, c, w1, b1, w2, b2, w3, b3, max_workgroups, &p)) return rc;
    if (W == 0 || H == 0) return SR_OK;
    if (!out) return fail(SR_ERR_INVALID_ARGUMENT, "sr_sky_forward: out is NULL");
    SR_HIP(launch_sky_forward(W, H, cam, p, max_workgroups, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_sky_backward(int32_t W, int32_t H, const float* cam, const float* w0sh, const float* c, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* w3, const float* b3, const float* g_out, int32_t max_workgroups, void* workspace,
                    size_t workspace_bytes, float* g_w0sh, float* g_c, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3,
                    void* stream) {
    SkyWeights p;
    if (int rc = sky_args("sr_sky_backward", W, H, cam, w0sh, c, w1, b1, w2, b2, w3, b3, max_workgroups, &p)) return rc;
    if (W == 0 || H == 0) return SR_OK;
    if (!g_out) return fail(SR_ERR_INVALID_ARGUMENT, "sr_sky_backward: g_out is NULL");
    float* const grads[8] = {g_w0sh, g_c, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
    bool any = false;
    for (float* g : grads) any = any || g != nullptr;
    if (!any) return SR_OK;
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "sr_sky_backward: workspace is NULL");
    if (workspace_bytes < sky_workspace_bytes(max_workgroups))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "sr_sky_backward: workspace %zu < %zu", workspace_bytes, sky_workspace_bytes(max_workgroups));
    SR_HIP(launch_sky_backward(W, H, cam, p, g_out, max_workgroups, workspace, grads, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_adam_step(const SrAdamSegment* segments, int32_t n_segments, double beta1, double beta2, double eps, void* stream) {
    if (!segments) return fail(SR_ERR_INVALID_ARGUMENT, "segments is NULL");
    if (n_segments < 1 || n_segments > SR_ADAM_MAX_SEGMENTS)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_segments %d not in 1..%d", n_segments, SR_ADAM_MAX_SEGMENTS);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta1 %g not in [0, 1)", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta2 %g not in [0, 1)", beta2);
    if (!(eps >= 0.0)) return fail(SR_ERR_INVALID_ARGUMENT, "eps %g is negative", eps);
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamSegment& a = segments[k];
        if (a.n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: n %lld is negative", k, (long long)a.n);
        const void* ptrs[4] = {a.param, a.grad, a.exp_avg, a.exp_avg_sq};
        const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int j = 0; j < 4; ++j) {
            if (!ptrs[j]) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is NULL", k, names[j]);
            if ((uintptr_t)ptrs[j] & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is not 4-B aligned", k, names[j]);
        }
    }
    if (!adam_supported(segments, n_segments)) return fail(SR_ERR_UNSUPPORTED, "the segments hold more than 2^31 chunks of %d elements", SR_ADAM_CHUNK);
    SR_HIP(launch_adam_step(segments, n_segments, beta1, beta2, eps, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_adam_step_rows(const SrAdamRowSegment* segments, int32_t n_segments, int32_t P, const uint8_t* mask, double beta1, double beta2,
                      double eps, void* stream) {
    if (!segments) return fail(SR_ERR_INVALID_ARGUMENT, "segments is NULL");
    if (n_segments < 1 || n_segments > SR_ADAM_MAX_SEGMENTS)
        return fail(SR_ERR_INVALID_ARGUMENT, "n_segments %d not in 1..%d", n_segments, SR_ADAM_MAX_SEGMENTS);
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P > 0 && !mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta1 %g not in [0, 1)", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(SR_ERR_INVALID_ARGUMENT, "beta2 %g not in [0, 1)", beta2);
    if (!(eps >= 0.0)) return fail(SR_ERR_INVALID_ARGUMENT, "eps %g is negative", eps);
    for (int k = 0; k < n_segments; ++k) {
        const SrAdamRowSegment& a = segments[k];
        if (a.row_len < 1 || a.row_len >= (1ll << 30)) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: row_len %lld not in [1, 2^30)", k, (long long)a.row_len);
        if (a.n != (int64_t)P * a.row_len)
            return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: n %lld is not P * row_len = %d * %lld", k, (long long)a.n, P, (long long)a.row_len);
        if (a.n == 0) continue;
        const void* ptrs[4] = {a.param, a.grad, a.exp_avg, a.exp_avg_sq};
        const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int j = 0; j < 4; ++j) {
            if (!ptrs[j]) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is NULL", k, names[j]);
            if ((uintptr_t)ptrs[j] & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "segment %d: %s is not 4-B aligned", k, names[j]);
        }
    }
    if (P == 0) return SR_OK;
    if (!adam_rows_supported(segments, n_segments)) return fail(SR_ERR_UNSUPPORTED, "the segments hold more than 2^31 chunks of %d elements", SR_ADAM_CHUNK);
    SR_HIP(launch_adam_step_rows(segments, n_segments, mask, beta1, beta2, eps, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

namespace {

// shared refusals of the two masked-model calls; *work = 0: nothing to do
int mask_model_args(int32_t P, int32_t sh_coeffs, const uint8_t* mask, uint32_t fixed_bits, int* work) {
    *work = 0;
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (sh_coeffs < 1) return fail(SR_ERR_INVALID_ARGUMENT, "sh_coeffs %d < 1", sh_coeffs);
    if (fixed_bits > 63u) return fail(SR_ERR_INVALID_ARGUMENT, "fixed_bits %u has bits beyond the six properties", fixed_bits);
    if (P == 0) return SR_OK;
    if (!mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    if (!mask_model_supported(P, sh_coeffs)) return fail(SR_ERR_UNSUPPORTED, "P * 3 * sh_coeffs = %d * 3 * %d reaches 2^31", P, sh_coeffs);
    *work = 1;
    return SR_OK;
}

int mask_pointer(const char* group, const char* name, const void* p, bool required) {
    if (!p && required) return fail(SR_ERR_INVALID_ARGUMENT, "%s.%s is NULL", group, name);
    if ((uintptr_t)p & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "%s.%s is not 4-B aligned", group, name);
    return SR_OK;
}

const char* const kMaskNames[6] = {"xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"};
const uint32_t kMaskBits[6] = {SR_MASK_FIXED_XYZ, SR_MASK_FIXED_FEATURES_DC, SR_MASK_FIXED_FEATURES_REST, SR_MASK_FIXED_OPACITY, SR_MASK_FIXED_SCALING,
                               SR_MASK_FIXED_ROTATION};

}  // namespace

int sr_mask_compose(int32_t P, int32_t sh_coeffs, const SrMaskTensors* base, const SrMaskTensors* delta, const uint8_t* mask,
                    uint32_t fixed_bits, const SrMaskEffective* out, void* stream) {
    int work;
    if (int rc = mask_model_args(P, sh_coeffs, mask, fixed_bits, &work)) return rc;
    if (!work) return SR_OK;
    if (!base || !delta || !out) return fail(SR_ERR_INVALID_ARGUMENT, "base / delta / out is NULL");
    const float* b[6] = {base->xyz, base->features_dc, base->features_rest, base->opacity, base->scaling, base->rotation};
    const float* d[6] = {delta->xyz, delta->features_dc, delta->features_rest, delta->opacity, delta->scaling, delta->rotation};
    for (int k = 0; k < 6; ++k) {
        const bool empty = k == 2 && sh_coeffs == 1;   // features_rest of SH degree 0
        if (int rc = mask_pointer("base", kMaskNames[k], b[k], !empty)) return rc;
        if (int rc = mask_pointer("delta", kMaskNames[k], d[k], !empty && !(fixed_bits & kMaskBits[k]))) return rc;
    }
    const uint32_t both = SR_MASK_FIXED_FEATURES_DC | SR_MASK_FIXED_FEATURES_REST;
    const float* o[5] = {out->xyz, out->features, out->opacity, out->scaling, out->rotation};
    const char* names[5] = {"xyz", "features", "opacity", "scaling", "rotation"};
    const bool fixed[5] = {(fixed_bits & SR_MASK_FIXED_XYZ) != 0, (fixed_bits & both) == both, (fixed_bits & SR_MASK_FIXED_OPACITY) != 0,
                           (fixed_bits & SR_MASK_FIXED_SCALING) != 0, (fixed_bits & SR_MASK_FIXED_ROTATION) != 0};
    for (int k = 0; k < 5; ++k)
        if (int rc = mask_pointer("out", names[k], o[k], !fixed[k])) return rc;
    SR_HIP(launch_mask_compose(P, sh_coeffs, *base, *delta, mask, fixed_bits, *out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_mask_compose_backward(int32_t P, int32_t sh_coeffs, const SrMaskEffective* upstream, const uint8_t* mask, uint32_t fixed_bits,
                             const SrMaskTensors* d_delta, void* stream) {
    int work;
    if (int rc = mask_model_args(P, sh_coeffs, mask, fixed_bits, &work)) return rc;
    if (!work) return SR_OK;
    if (!upstream || !d_delta) return fail(SR_ERR_INVALID_ARGUMENT, "upstream / d_delta is NULL");
    const float* d[6] = {d_delta->xyz, d_delta->features_dc, d_delta->features_rest, d_delta->opacity, d_delta->scaling, d_delta->rotation};
    const float* g[6] = {upstream->xyz, upstream->features, upstream->features, upstream->opacity, upstream->scaling, upstream->rotation};
    const char* from[6] = {"xyz", "features", "features", "opacity", "scaling", "rotation"};
    for (int k = 0; k < 6; ++k) {
        if (int rc = mask_pointer("d_delta", kMaskNames[k], d[k], false)) return rc;
        if (int rc = mask_pointer("upstream", from[k], g[k], false)) return rc;
        if (!d[k] || (k == 2 && sh_coeffs == 1)) continue;
        if (fixed_bits & kMaskBits[k]) return fail(SR_ERR_INVALID_ARGUMENT, "d_delta.%s is asked for, but the property is fixed", kMaskNames[k]);
        if (!g[k]) return fail(SR_ERR_INVALID_ARGUMENT, "d_delta.%s is asked for without upstream.%s", kMaskNames[k], from[k]);
    }
    SR_HIP(launch_mask_compose_backward(P, sh_coeffs, *upstream, mask, *d_delta, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_densification_stats(int32_t P, const float* viewspace_grad, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                           float* max_radii2D, void* stream) {
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P == 0) return SR_OK;
    if (!viewspace_grad) return fail(SR_ERR_INVALID_ARGUMENT, "viewspace_grad is NULL");
    if (!radii) return fail(SR_ERR_INVALID_ARGUMENT, "radii is NULL");
    if (!xyz_gradient_accum) return fail(SR_ERR_INVALID_ARGUMENT, "xyz_gradient_accum is NULL");
    if (!denom) return fail(SR_ERR_INVALID_ARGUMENT, "denom is NULL");
    if (!max_radii2D) return fail(SR_ERR_INVALID_ARGUMENT, "max_radii2D is NULL");
    if (((uintptr_t)viewspace_grad | (uintptr_t)radii | (uintptr_t)xyz_gradient_accum | (uintptr_t)denom | (uintptr_t)max_radii2D) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "viewspace_grad / radii / xyz_gradient_accum / denom / max_radii2D: a pointer is not 4-B aligned");
    SR_HIP(launch_densification_stats(P, viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

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
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < densify_workspace_bytes(P))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, densify_workspace_bytes(P));
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
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
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < densify_workspace_bytes(P))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, densify_workspace_bytes(P));
    SR_HIP(densify_apply(P, counts, noise, rotation, scaling, segments, n_segments, workspace, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

// the checks sr_tsdf_fuse and sr_tsdf_fuse_grid share -> the kernels' view of the arguments
static int tsdf_arguments(const SrTsdfViews* views, const SrTsdfSpace* space, long long n, const float* tsdf, const float* rgb, TsdfViewsDev* v,
                          TsdfSpace* sp) {
    if (!views || !space) return fail(SR_ERR_INVALID_ARGUMENT, "views / space is NULL");
    if (!views->maps) return fail(SR_ERR_INVALID_ARGUMENT, "maps is NULL");
    if (!views->full_proj) return fail(SR_ERR_INVALID_ARGUMENT, "full_proj is NULL");
    if (views->V < 1) return fail(SR_ERR_INVALID_ARGUMENT, "V = %d: at least one view", views->V);
    if (views->H < 2 || views->W < 2) return fail(SR_ERR_INVALID_ARGUMENT, "maps of %d x %d: H and W must be at least 2", views->H, views->W);
    if (views->channels != 1 && views->channels != 4) return fail(SR_ERR_INVALID_ARGUMENT, "channels = %d: 1 (depth) or 4 (depth, r, g, b)", views->channels);
    if ((uintptr_t)views->maps & (views->channels == 4 ? 15u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "maps is not %d-B aligned", 4 * views->channels);
    if ((uintptr_t)views->full_proj & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "full_proj is not 4-B aligned");
    if (!(space->voxel_size > 0.0)) return fail(SR_ERR_INVALID_ARGUMENT, "voxel_size = %g: must be positive", space->voxel_size);
    if (rgb && views->channels != 4) return fail(SR_ERR_INVALID_ARGUMENT, "rgb asked for, but the maps hold depths only (channels = 1)");
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n < 0");
    if (n >= (1ll << 31)) return fail(SR_ERR_UNSUPPORTED, "%lld samples in one call: fewer than 2^31 (split the call)", n);
    if (n > 0 && !tsdf) return fail(SR_ERR_INVALID_ARGUMENT, "tsdf is NULL");
    *v = TsdfViewsDev{views->maps, views->full_proj, views->V, views->H, views->W, views->channels};
    *sp = TsdfSpace{(float)(5.0 * space->voxel_size), space->contract ? 1 : 0, {space->center[0], space->center[1], space->center[2]}, space->radius};
    return SR_OK;
}

int sr_tsdf_fuse(const SrTsdfViews* views, const SrTsdfSpace* space, int32_t n, const float* samples, float* tsdf, float* rgb, float* weight,
                 void* stream) {
    TsdfViewsDev v; TsdfSpace sp;
    if (int rc = tsdf_arguments(views, space, n, tsdf, rgb, &v, &sp)) return rc;
    if (n == 0) return SR_OK;
    if (!samples) return fail(SR_ERR_INVALID_ARGUMENT, "samples is NULL");
    SR_HIP(launch_tsdf_fuse(v, sp, nullptr, n, samples, tsdf, rgb, weight, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_tsdf_fuse_grid(const SrTsdfViews* views, const SrTsdfSpace* space, const int32_t* dims, const float* lo, const float* step,
                      int32_t ix_begin, int32_t ix_end, float* tsdf, float* rgb, float* weight, void* stream) {
    if (!dims || !lo || !step) return fail(SR_ERR_INVALID_ARGUMENT, "dims / lo / step is NULL");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(SR_ERR_INVALID_ARGUMENT, "dims %d x %d x %d: every axis holds at least one sample", dims[0], dims[1], dims[2]);
    if (ix_begin < 0 || ix_end < ix_begin || ix_end > dims[0]) return fail(SR_ERR_INVALID_ARGUMENT, "slab [%d, %d) is not inside [0, %d)", ix_begin, ix_end, dims[0]);
    if ((long long)dims[1] * dims[2] >= (1ll << 31)) return fail(SR_ERR_UNSUPPORTED, "one plane of %d x %d samples: fewer than 2^31", dims[1], dims[2]);
    const long long n = (long long)(ix_end - ix_begin) * dims[1] * dims[2];
    TsdfViewsDev v; TsdfSpace sp;
    if (int rc = tsdf_arguments(views, space, n, tsdf, rgb, &v, &sp)) return rc;
    if (n == 0) return SR_OK;
    const TsdfGrid g{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, dims[1], dims[2], ix_begin};
    SR_HIP(launch_tsdf_fuse(v, sp, &g, (int)n, nullptr, tsdf, rgb, weight, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

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
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < mesh_workspace_bytes((uint32_t)n)) return fail(SR_ERR_INVALID_ARGUMENT, "workspace %zu < %zu", workspace_bytes, mesh_workspace_bytes((uint32_t)n));
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    if ((uintptr_t)volume & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "volume is not 4-B aligned");
    *g = MeshGrid{dims[0], dims[1], dims[2], (uint32_t)n, level};
    *cells = dims[0] > 1 && dims[1] > 1 && dims[2] > 1;
    return SR_OK;
}

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

// the checks the three sr_mesh_* post-processing calls share; *work = 0 for a mesh without faces or without vertices
static int mesh_post_arguments(const int32_t* faces, int32_t nv, int32_t nf, const void* workspace, size_t workspace_bytes, bool* work) {
    if (nv < 0 || nf < 0) return fail(SR_ERR_INVALID_ARGUMENT, "nv %d / nf %d is negative", nv, nf);
    if (nf > 0x7FFFFFFF / 3) return fail(SR_ERR_UNSUPPORTED, "%d faces: 3 nf does not fit in int32 (process the mesh in parts)", nf);
    *work = nv > 0 && nf > 0;
    if (!*work) return SR_OK;
    if (!faces) return fail(SR_ERR_INVALID_ARGUMENT, "faces is NULL");
    if ((uintptr_t)faces & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "faces is not 4-B aligned");
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < mesh_post_workspace_bytes(nv, nf))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, mesh_post_workspace_bytes(nv, nf));
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    return SR_OK;
}

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

// the checks the per-point sr_* calls of unveil.hip share; *work = 0 where there is no point or no frame
static int unveil_point_arguments(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, bool* work) {
    if (P < 0 || F < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P %d / F %d is negative", P, F);
    *work = P > 0 && F > 0;
    if (!*work) return SR_OK;
    if (!xyz || !cams || !hw) return fail(SR_ERR_INVALID_ARGUMENT, "xyz / cams / hw is NULL");
    if (((uintptr_t)xyz | (uintptr_t)cams | (uintptr_t)hw) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "xyz / cams / hw is not 4-B aligned");
    return SR_OK;
}

static int unveil_workspace(int32_t P, int32_t F, const void* workspace, size_t workspace_bytes) {
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < unveil_workspace_bytes(P, F)) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, unveil_workspace_bytes(P, F));
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    return SR_OK;
}

// the checks the per-pixel sr_* calls of unveil.hip share
static int unveil_image_arguments(int32_t H, int32_t W, int32_t k) {
    if (H < 1 || W < 1) return fail(SR_ERR_INVALID_ARGUMENT, "an image of %d x %d: H and W must be at least 1", H, W);
    if ((long long)H * W > 0x7FFFFFFFll) return fail(SR_ERR_UNSUPPORTED, "an image of %d x %d: H W must fit in int32", H, W);
    // a tile is 64 x kDilateRows pixels: the tile rows are the launch's grid.y, and a tile's halo reaches 64 columns past its own
    if (H > kDilateRows * 65535) return fail(SR_ERR_UNSUPPORTED, "an image of %d rows: at most %d", H, kDilateRows * 65535);
    if (W > 0x7FFFFFFF - 128) return fail(SR_ERR_UNSUPPORTED, "an image of %d columns: at most %d", W, 0x7FFFFFFF - 128);
    if (k < 1 || k > 31) return fail(SR_ERR_INVALID_ARGUMENT, "k = %d not in 1..31", k);
    return SR_OK;
}

size_t sr_unveil_workspace_bytes(int32_t P, int32_t F) {
    if (P < 0 || F < 0) return 0;
    return unveil_workspace_bytes(P, F);
}

int sr_points_in_frame(int32_t P, const float* xyz, const float* cam, const int32_t* hw, uint8_t* mask, void* workspace, size_t workspace_bytes,
                       uint32_t* count, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, 1, xyz, cam, hw, &work)) return rc;
    if ((uintptr_t)count & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "count is not 4-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {
        if (count) SR_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
        return SR_OK;
    }
    if (!mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    if (count) if (int rc = unveil_workspace(P, 1, workspace, workspace_bytes)) return rc;
    SR_HIP(points_in_frame(P, xyz, cam, hw, mask, workspace, count, s));
    return SR_OK;
}

int sr_points_in_frame_emit(int32_t P, const float* xyz, const float* cam, const int32_t* hw, void* workspace, size_t workspace_bytes, int32_t n,
                            int64_t* pix, float* depth, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, 1, xyz, cam, hw, &work)) return rc;
    if (n < 0 || n > P) return fail(SR_ERR_INVALID_ARGUMENT, "n = %d: not in 0..P = %d", n, P);
    if (n == 0) return SR_OK;
    if (int rc = unveil_workspace(P, 1, workspace, workspace_bytes)) return rc;
    if (!pix || !depth) return fail(SR_ERR_INVALID_ARGUMENT, "pix / depth is NULL");
    if (((uintptr_t)pix & 7u) || ((uintptr_t)depth & 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "pix is not 8-B or depth not 4-B aligned");
    SR_HIP(points_in_frame_emit(P, xyz, cam, hw, workspace, (uint32_t)n, pix, depth, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_frame_visibility(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, void* workspace, size_t workspace_bytes,
                        int64_t* count, double* depth_sum, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, F, xyz, cams, hw, &work)) return rc;
    if (F == 0) return SR_OK;
    if (!count || !depth_sum) return fail(SR_ERR_INVALID_ARGUMENT, "count / depth_sum is NULL");
    if (((uintptr_t)count | (uintptr_t)depth_sum) & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "count / depth_sum is not 8-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {   // no point: every count and sum is 0 (all bits zero)
        SR_HIP(hipMemsetAsync(count, 0, sizeof(int64_t) * (size_t)F, s));
        SR_HIP(hipMemsetAsync(depth_sum, 0, sizeof(double) * (size_t)F, s));
        return SR_OK;
    }
    if (int rc = unveil_workspace(P, F, workspace, workspace_bytes)) return rc;
    SR_HIP(frame_visibility(P, F, xyz, cams, hw, workspace, count, depth_sum, s));
    return SR_OK;
}

int sr_semantic_mask_of_points(int32_t P, int32_t F, const float* xyz, const float* cams, const int32_t* hw, const uint8_t* maps, int32_t Hm,
                               int32_t Wm, uint32_t remain_bit, uint8_t* mask, uint64_t* n_out_of_range, void* stream) {
    bool work;
    if (int rc = unveil_point_arguments(P, F, xyz, cams, hw, &work)) return rc;
    if (Hm < 1 || Wm < 1) return fail(SR_ERR_INVALID_ARGUMENT, "maps of %d x %d: Hm and Wm must be at least 1", Hm, Wm);
    if (!n_out_of_range) return fail(SR_ERR_INVALID_ARGUMENT, "n_out_of_range is NULL");
    if ((uintptr_t)n_out_of_range & 7u) return fail(SR_ERR_INVALID_ARGUMENT, "n_out_of_range is not 8-B aligned");
    if (P > 0 && !mask) return fail(SR_ERR_INVALID_ARGUMENT, "mask is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!work) {   // no frame sets anything
        SR_HIP(hipMemsetAsync(n_out_of_range, 0, sizeof(uint64_t), s));
        if (P > 0) SR_HIP(hipMemsetAsync(mask, 0, (size_t)P, s));
        return SR_OK;
    }
    if (!maps) return fail(SR_ERR_INVALID_ARGUMENT, "maps is NULL");
    const UnveilSemantic a{P, F, Hm, Wm, remain_bit & 0x7FFFFFFFu, xyz, cams, hw, maps};
    SR_HIP(semantic_mask_of_points(a, mask, n_out_of_range, s));
    return SR_OK;
}

int sr_dilate_mask(int32_t H, int32_t W, int32_t k, const uint8_t* mask, uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!mask || !out) return fail(SR_ERR_INVALID_ARGUMENT, "mask / out is NULL");
    if (mask == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the mask: a tile reads its neighbours' pixels");
    SR_HIP(dilate_mask(H, W, k, mask, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_instance_pixel_mask(int32_t H, int32_t W, const float* alpha_a, const float* alpha_b, float threshold, int32_t k, uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!alpha_a || !alpha_b || !out) return fail(SR_ERR_INVALID_ARGUMENT, "alpha_a / alpha_b / out is NULL");
    if (((uintptr_t)alpha_a | (uintptr_t)alpha_b) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "alpha_a / alpha_b is not 4-B aligned");
    if (threshold != threshold) return fail(SR_ERR_INVALID_ARGUMENT, "threshold is NaN");
    SR_HIP(instance_pixel_mask(H, W, k, alpha_a, alpha_b, threshold, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_refill_mask(int32_t H, int32_t W, int32_t C, const float* render_a, const float* render_b, const uint8_t* mask, float eps, int32_t k,
                   uint8_t* out, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (C < 1 || C > 16) return fail(SR_ERR_UNSUPPORTED, "C = %d channels: 1..16", C);
    if (!render_a || !render_b || !mask || !out) return fail(SR_ERR_INVALID_ARGUMENT, "render_a / render_b / mask / out is NULL");
    if (mask == out) return fail(SR_ERR_INVALID_ARGUMENT, "out must not be the mask: a tile reads its neighbours' pixels");
    if (((uintptr_t)render_a | (uintptr_t)render_b) & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "render_a / render_b is not 4-B aligned");
    if (eps != eps) return fail(SR_ERR_INVALID_ARGUMENT, "eps is NaN");
    SR_HIP(refill_mask(H, W, C, k, render_a, render_b, mask, eps, out, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_inpaint_conditions(int32_t H, int32_t W, const float* full_render, const float* full_alpha, const float* background_render,
                          const float* background_alpha, const float* background_depth, const float* background_normal, const float* sky,
                          float threshold, int32_t k, uint8_t* mask, uint8_t* original_rgb, uint8_t* inpainted_rgb, uint8_t* empty_opacity,
                          uint8_t* inpainted_depth, uint8_t* inpainted_normal, void* stream) {
    if (int rc = unveil_image_arguments(H, W, k)) return rc;
    if (!full_render || !full_alpha || !background_render || !background_alpha || !background_depth || !background_normal || !sky)
        return fail(SR_ERR_INVALID_ARGUMENT, "an input image is NULL");
    if (((uintptr_t)full_render | (uintptr_t)full_alpha | (uintptr_t)background_render | (uintptr_t)background_alpha | (uintptr_t)background_depth |
         (uintptr_t)background_normal | (uintptr_t)sky) & 3u)
        return fail(SR_ERR_INVALID_ARGUMENT, "an input image is not 4-B aligned");
    if (!mask || !original_rgb || !inpainted_rgb || !empty_opacity || !inpainted_depth || !inpainted_normal)
        return fail(SR_ERR_INVALID_ARGUMENT, "an output is NULL");
    if (threshold != threshold) return fail(SR_ERR_INVALID_ARGUMENT, "threshold is NaN");
    const UnveilConditions a{H, W, full_render, full_alpha, background_render, background_alpha, background_depth, background_normal, sky,
                             original_rgb, inpainted_rgb, empty_opacity, inpainted_depth, inpainted_normal};
    SR_HIP(inpaint_conditions(a, threshold, k, mask, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

// the checks the three launching sr_voxel_* calls share: the cloud and the workspace
static int voxel_arguments(int32_t n, const void* points, int32_t points_f64, const void* workspace, size_t workspace_bytes) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n %d is negative", n);
    if (points_f64 != 0 && points_f64 != 1) return fail(SR_ERR_INVALID_ARGUMENT, "points_f64 = %d: 0 (float32) or 1 (float64)", points_f64);
    if (n == 0) return SR_OK;
    if (!points) return fail(SR_ERR_INVALID_ARGUMENT, "points is NULL");
    if ((uintptr_t)points & (points_f64 ? 7u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "points is not aligned to its element size");
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if (workspace_bytes < voxel_workspace_bytes((uint32_t)n))
        return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, voxel_workspace_bytes((uint32_t)n));
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    return SR_OK;
}

static int voxel_attribute(const char* name, const void* p, int32_t is_f64) {
    if (is_f64 != 0 && is_f64 != 1) return fail(SR_ERR_INVALID_ARGUMENT, "%s_f64 = %d: 0 (float32) or 1 (float64)", name, is_f64);
    if ((uintptr_t)p & (is_f64 ? 7u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "%s is not aligned to its element size", name);
    return SR_OK;
}

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
    if (int rc = voxel_attribute("colors", colors, colors_f64)) return rc;
    if (int rc = voxel_attribute("normals", normals, normals_f64)) return rc;
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

// the checks the three launching sr_lidar_* calls share: the cloud, the view table and the workspace of n * rows_per_point rows
static int lidar_arguments(int32_t n, const void* points, int32_t points_f64, const void* views, int32_t n_views, const uint8_t* label_lut,
                           int32_t rows_per_point, const void* workspace, size_t workspace_bytes, bool needs_views) {
    if (n < 0) return fail(SR_ERR_INVALID_ARGUMENT, "n %d is negative", n);
    if (points_f64 != 0 && points_f64 != 1) return fail(SR_ERR_INVALID_ARGUMENT, "points_f64 = %d: 0 (float32) or 1 (float64)", points_f64);
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
    if ((uintptr_t)points & (points_f64 ? 7u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "points is not aligned to its element size");
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is NULL");
    const size_t need = lidar_label_workspace_bytes((uint64_t)n * (uint64_t)rows_per_point);
    if (workspace_bytes < need) return fail(SR_ERR_BUFFER_TOO_SMALL, "workspace %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    return SR_OK;
}

static int lidar_sweeps(int32_t n, const int32_t* sweep_offsets, int32_t n_sweeps, int32_t max_sweep_points) {
    if (n_sweeps < 1 || n_sweeps > kLabelMaxViews) return fail(SR_ERR_INVALID_ARGUMENT, "n_sweeps = %d: 1..%d", n_sweeps, kLabelMaxViews);
    if ((uintptr_t)sweep_offsets & 3u) return fail(SR_ERR_INVALID_ARGUMENT, "sweep_offsets is not 4-B aligned");
    if (!sweep_offsets && n_sweeps != 1) return fail(SR_ERR_INVALID_ARGUMENT, "sweep_offsets is NULL with %d sweeps", n_sweeps);
    if (max_sweep_points < 0 || max_sweep_points > n) return fail(SR_ERR_INVALID_ARGUMENT, "max_sweep_points = %d: not in 0..n = %d", max_sweep_points, n);
    if (n > 0 && max_sweep_points < 1) return fail(SR_ERR_INVALID_ARGUMENT, "max_sweep_points = 0 with %d points", n);
    return SR_OK;
}

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

int sr_debug_lds_atomic_ranks(const uint32_t* digits, uint32_t* ranks, uint32_t n, int bins, void* stream) {
    if (n > 0 && (!digits || !ranks)) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (bins < 1 || bins > 1024 || (n % 256u) != 0u) return fail(SR_ERR_INVALID_ARGUMENT, "bins %d not in 1..1024 or n %u not a multiple of 256", bins, n);
    SR_HIP(lds_atomic_ranks(digits, ranks, n, bins, static_cast<hipStream_t>(stream)));
    return SR_OK;
}

int sr_rank_mode(void* stream) {
    RankMode mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), false, &mode)) return rc;
    return (int)mode;
}

size_t sr_debug_radix_sort_temp_bytes(uint32_t n) { return radix_sort_temp_bytes(n); }

int sr_debug_radix_sort(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t n,
                        int total_bits, void* temp, size_t temp_bytes, uint32_t flags, void* stream) {
    if (n > 0 && (!keys_in || !keys_out || !vals_out || !temp)) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (total_bits < 1 || total_bits > 32) return fail(SR_ERR_INVALID_ARGUMENT, "total_bits %d not in 1..32", total_bits);
    if (temp_bytes < radix_sort_temp_bytes(n)) return fail(SR_ERR_BUFFER_TOO_SMALL, "temp %zu < %zu", temp_bytes, radix_sort_temp_bytes(n));
    RankMode sort_mode = kRankUnknown;
    if (int rc = rank_mode(static_cast<hipStream_t>(stream), (flags & SR_FLAG_BALLOT_RANKING) != 0, &sort_mode)) return rc;
    SR_HIP(radix_sort_pairs(keys_in, vals_in, keys_out, vals_out, n, total_bits, temp, temp_bytes, static_cast<hipStream_t>(stream), nullptr, nullptr, sort_mode,
                            (flags & SR_FLAG_ONE_SWEEP_SORT) != 0));
    return SR_OK;
}

void sr_set_stage_timing(int enable) {
    std::lock_guard<std::mutex> lk(g_ring_mu);
    g_timing.store(enable);
    if (enable) for (auto& r : g_ring) r.used = 0;
}

int sr_stage_stats(int stage, float* total_ms, int* launches) {
    if (stage < 0 || stage >= SR_STAGE_COUNT || !total_ms || !launches) return fail(SR_ERR_INVALID_ARGUMENT, "bad stage / NULL output");
    std::lock_guard<std::mutex> lk(g_ring_mu);
    EvRing& r = g_ring[stage];
    float sum = 0.f;
    int done = 0;
    for (int i = 0; i < r.used; ++i) {
        if (!r.closed[i]) continue;
        ++done;
        float ms = 0.f;
        SR_HIP(hipEventSynchronize(r.ev[i][1]));
        SR_HIP(hipEventElapsedTime(&ms, r.ev[i][0], r.ev[i][1]));
        sum += ms;
    }
    *total_ms = sum;
    *launches = done;
    return SR_OK;
}

}  // extern "C"
