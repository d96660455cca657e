// api.hip -- the rasteriser's part of the C-ABI (include/surfel_raster.h): its state-buffer layouts, argument checks, blend choice and stage
// sequencing; the class passes; the debug and timing entry points; and what every entry point of the library shares (abi.h): the error
// text, the per-device ranking mode, the per-thread pinned words.  The entry points of a stand-alone op sit at the end of its own file.
// Every rasteriser entry point resolves (frame, g) and its state buffers through one Call; it keeps its own checks, early-outs and stages.
// No torch types, no exceptions across the boundary, nothing allocated persistently.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <atomic>
#include <mutex>

#include "abi.h"

using namespace sr;

namespace {

thread_local char g_err[512] = "";
// The only process-wide state of the library is this profiling aid (everything that changes what a call does is a field
// of that call's SrFrame): autograd runs the backward on its own thread, so the rings are shared and mutex-protected.
std::atomic<int> g_timing{0};
std::mutex g_ring_mu;

}  // namespace

int sr::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

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

}  // namespace

// ---- what abi.h declares ---------------------------------------------------------------------------------------------------------
// One 64-B pinned host block per calling thread (with one event per (thread, device) the only things this library keeps): word 0 =
// the DMA target of the num_rendered read-back, words 4..7 = the four counts of sr_densify_plan, word 8 = the result word of the rank
// self-check.
// (portable + mapped: valid on every device of the process, whichever is current when the thread first calls in.  Never freed: 64 B per
// calling thread, and a destructor at thread / process exit could run after the HIP runtime has been torn down.)
uint32_t* sr::pinned_words() {
    static thread_local uint32_t* pinned = nullptr;
    if (!pinned && hipHostMalloc(reinterpret_cast<void**>(&pinned), 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { pinned = nullptr; (void)hipGetLastError(); }
    return pinned;
}

// The device a stream belongs to (the cache below is per device: the CURRENT device may be another one); the null stream -> current device.
int sr::stream_device(hipStream_t s, int* dev) {
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
namespace {
constexpr int kMaxDevices = 64;
std::atomic<int> g_rank_mode[kMaxDevices];
}  // namespace
int sr::rank_mode(hipStream_t s, bool force_ballot, RankMode* mode) {
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

namespace {

// ---- buffer layouts ------------------------------------------------------------------------------
// A layout = the byte offsets of a state buffer's regions (every region 256-B aligned) + its total; a view = the typed pointers of one
// buffer carved by that layout.  A call carves each buffer once, in Call::bind below (launch.h: Carver, at<T>).
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
WorkspaceView workspace_view(void* workspace, const WorkspaceLayout& L) {
    return WorkspaceView{at<float4>(workspace, L.records), at<uint8_t>(workspace, L.written)};
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
struct ClassView {
    float* state; uint32_t* last; uint32_t* tile_total; uint2* ranges;
    uint8_t* ids; uint16_t* hit;   // of the class-shared state alone (below); nullptr in a class image
};
ClassView class_view(void* class_image, const ClassLayout& L) {
    return ClassView{at<float>(class_image, L.state), at<uint32_t>(class_image, L.last), at<uint32_t>(class_image, L.tile_total), at<uint2>(class_image, L.ranges),
                     nullptr, nullptr};
}

// The state of the per-class pass on the binning of a colour pass (sr_class_*_shared): a class image + what the colour pass keeps for itself.
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
ClassView class_shared_view(void* class_state, const ClassSharedLayout& L) {
    ClassView C = class_view(class_state, L.C);
    C.ids = at<uint8_t>(class_state, L.ids); C.hit = at<uint16_t>(class_state, L.hit);
    return C;
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
// what the per-Gaussian backward kernels read of the geometry state (`with_sh_jac` false: the class pass on a colour pass's binning, whose
// sh_jac region is the colour pass's)
void set_backward_state(FrameDev* f, const SrFrame* frame, const GeomView& G, bool with_sh_jac) {
    f->first = G.first; f->first_base = G.block_base;
    if (with_sh_jac) f->sh_jac = G.sh_jac;
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

// ---- one call's arguments, resolved once ---------------------------------------------------------------------------------------------
// The two refusals of a caller's buffer; each text stands here and nowhere else.
enum BufferKind { kGeom, kBinning, kImage, kClassImage, kClassState, kWorkspace };
int check_present(BufferKind kind, const void* p) {
    static const char* const text[] = {"geom is NULL", "binning is NULL", "image is NULL", "class_image is NULL", "class_state is NULL", "workspace is NULL"};
    return p ? SR_OK : fail(SR_ERR_INVALID_ARGUMENT, "%s", text[kind]);
}
int check_size(BufferKind kind, size_t have, size_t need) {
    static const char* const text[] = {"geom buffer %zu < %zu", "binning buffer %zu < %zu", "image buffer %zu < %zu",
                                       "class image buffer %zu < %zu", "class state buffer %zu < %zu", "workspace %zu < %zu"};
    return have >= need ? SR_OK : fail(SR_ERR_BUFFER_TOO_SMALL, text[kind], have, need);
}

// The buffers an entry point asks bind() for, named where it asks; `wanted` false: not needed in this call.  cls: the class image, or the
// class-shared state where the call's ClassPass has the ids in an array of their own.  channels: of the workspace's gradient records.
struct Raw { void* p = nullptr; size_t bytes = 0; bool wanted = false; };
struct Buffers {
    Raw geom_, binning_, image_, cls_, workspace_; int channels_ = 0;
    Buffers& geom(void* p, size_t n, bool wanted = true) { geom_ = Raw{p, n, wanted}; return *this; }
    Buffers& binning(void* p, size_t n) { binning_ = Raw{p, n, true}; return *this; }
    Buffers& image(void* p, size_t n, bool wanted = true) { image_ = Raw{p, n, wanted}; return *this; }
    Buffers& cls(void* p, size_t n) { cls_ = Raw{p, n, true}; return *this; }
    Buffers& workspace(void* p, size_t n, int channels) { workspace_ = Raw{p, n, true}; channels_ = channels; return *this; }
};
// Where bind() looks at the geometry buffer: before the call's other buffers (the backward calls and sr_debug_pair_decisions), or after
// all of them (the forward calls, which did so inside bin_duplicates).  Each entry point keeps the order it had; the two are not unified.
enum class GeomOrder { kFirst, kLast };

// The checks of (frame, g): check_common alone; with choose_blend (the colour pass's calls that blend); check_class_pass with a ClassPass.
enum class Checks { kCommon, kBlend, kClassPass };
struct ClassPass { int n_classes = 0; ClassIds ids = ClassIds::kInColors; bool refuse_transmat = false; };

// What an entry point works with, in two steps because its own argument checks and P == 0 / D == 0 early-outs lie between them: open()
// checks (frame, g) and fills P, f, blend and s; bind() checks the buffers the call needs and carves their views, each layout computed
// once and each view carved from the layout its size was checked against.  The views of a buffer that was not bound stay NULL.
struct Call {
    const SrFrame* frame; const SrGaussians* g; bool backward; ClassPass cp;
    int P; FrameDev f; BlendChoice blend; hipStream_t s;
    GeomLayout GL;   // (the scan and the sort take region sizes of it)
    GeomView G; BinView B; ImgView I; ClassView C; WorkspaceView ws;

    int open(const SrFrame* frame_, const SrGaussians* g_, Checks checks, bool backward_, void* stream, ClassPass cp_ = ClassPass{}) {
        frame = frame_; g = g_; backward = backward_; cp = cp_;
        if (int rc = checks == Checks::kClassPass ? check_class_pass(frame, g, cp.n_classes, cp.ids, cp.refuse_transmat) : check_common(frame, g)) return rc;
        if (backward) if (int rc = check_backward_frame(frame)) return rc;
        P = g->P; f = make_frame(frame, g); s = static_cast<hipStream_t>(stream);
        return checks == Checks::kBlend ? choose_blend(frame, f, !backward, &blend) : SR_OK;
    }

    // Within one look the NULL buffers are refused before the short ones, each in argument order, as every entry point did.
    int bind(uint32_t D, GeomOrder geom_order, const Buffers& b) {
        const bool shared = cp.ids == ClassIds::kOwnArray;
        const BinLayout BL = b.binning_.wanted ? bin_layout(D, f.W, f.H) : BinLayout{};
        const ImgLayout IL = b.image_.wanted ? img_layout(f.W, f.H) : ImgLayout{};
        const ClassLayout CL = b.cls_.wanted && !shared ? class_layout(f.W, f.H, cp.n_classes) : ClassLayout{};
        const ClassSharedLayout SL = b.cls_.wanted && shared ? class_shared_layout(P, f.W, f.H, cp.n_classes, D) : ClassSharedLayout{};
        const WorkspaceLayout WL = b.workspace_.wanted ? workspace_layout(D, b.channels_) : WorkspaceLayout{};
        if (b.geom_.wanted) GL = geom_layout(P);
        const struct { const Raw& raw; BufferKind kind; size_t need; } all[] = {
            {b.geom_, kGeom, GL.total}, {b.binning_, kBinning, BL.total}, {b.image_, kImage, IL.total},
            {b.cls_, shared ? kClassState : kClassImage, shared ? SL.total : CL.total}, {b.workspace_, kWorkspace, WL.total}};
        auto refusal = [&](int from, int to) {   // of all[from, to): the first NULL one, else the first short one
            for (int i = from; i < to; ++i) if (all[i].raw.wanted) if (int rc = check_present(all[i].kind, all[i].raw.p)) return rc;
            for (int i = from; i < to; ++i) if (all[i].raw.wanted) if (int rc = check_size(all[i].kind, all[i].raw.bytes, all[i].need)) return rc;
            return (int)SR_OK;
        };
        if (int rc = refusal(geom_order == GeomOrder::kFirst ? 0 : 1, 5)) return rc;
        if (geom_order == GeomOrder::kLast) if (int rc = refusal(0, 1)) return rc;
        if (b.geom_.wanted) G = geom_view(b.geom_.p, GL);
        if (b.binning_.wanted) B = bin_view(b.binning_.p, BL);
        if (b.image_.wanted) I = img_view(b.image_.p, IL);
        if (b.cls_.wanted) C = shared ? class_shared_view(b.cls_.p, SL) : class_view(b.cls_.p, CL);
        if (b.workspace_.wanted) ws = workspace_view(b.workspace_.p, WL);
        if (backward && b.geom_.wanted) set_backward_state(&f, frame, G, !shared);
        return SR_OK;
    }
};

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
    if (int rc = check_size(kGeom, geom_bytes, L.total)) return rc;
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
    if (int rc = check_size(kBinning, binning_bytes, L.total)) return rc;
    const BinView B = bin_view(binning, L);
    out->point_list = B.point_list;
    out->ranges = reinterpret_cast<uint32_t*>(B.ranges); out->tile_order = B.order;
    return SR_OK;
}

int sr_image_view(void* image, size_t image_bytes, int32_t W, int32_t H, SrImageView* out) {
    if (!image || !out) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    const ImgLayout L = img_layout(W, H);
    if (int rc = check_size(kImage, image_bytes, L.total)) return rc;
    const ImgView I = img_view(image, L);
    out->final_T = I.final_T; out->n_contrib = I.n_contrib;
    return SR_OK;
}

int sr_forward_plan(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, int32_t* radii,
                    uint32_t* num_rendered_host, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kCommon, false, stream)) return rc;
    if (!num_rendered_host) return fail(SR_ERR_INVALID_ARGUMENT, "num_rendered_host is NULL");
    *num_rendered_host = 0;
    const int P = c.P;
    if (P == 0) return SR_OK;
    if (!geom || !radii) return fail(SR_ERR_INVALID_ARGUMENT, "geom / radii is NULL");
    if (int rc = c.bind(0, GeomOrder::kLast, Buffers{}.geom(geom, geom_bytes))) return rc;
    const GeomLayout& L = c.GL; const GeomView& G = c.G; hipStream_t s = c.s; FrameDev& f = c.f;
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
// K3..K5 (duplicate emission, tile partition, tile ranges + dispatch order): shared by the blend forward and the per-class pass.  The call
// has bound its binning buffer and, where there is anything to bin (P > 0 and D > 0), its geometry buffer.
int bin_duplicates(const Call& c, uint32_t D) {
    const SrFrame* frame = c.frame; const FrameDev& f = c.f; hipStream_t s = c.s;
    const GeomLayout& L = c.GL; const GeomView& G = c.G; const BinView& B = c.B;
    const int P = c.P, n_tiles = f.tiles_x * f.tiles_y;
    if (P > 0 && D > 0) {
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
}  // namespace

int sr_forward_render(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning,
                      size_t binning_bytes, void* image, size_t image_bytes, uint32_t D, float* out_color,
                      float* out_allmap, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kBlend, false, stream)) return rc;
    const bool fwd_only = (frame->flags & SR_FLAG_FORWARD_ONLY) != 0;   // no backward follows: its state (image buffer, hit masks) is not written
    if (!binning || (!image && !fwd_only) || !out_color || !out_allmap) return fail(SR_ERR_INVALID_ARGUMENT, "binning / image / out_color / out_allmap is NULL");
    // The geometry buffer: needed where there is anything to bin; otherwise taken (and then checked like any other) if the caller gives one,
    // for the frame counts the emission scan left in it -- which the device-picked kernel reads, so that kernel insists on it.
    const bool binned = c.P > 0 && D > 0;
    if (int rc = c.bind(D, GeomOrder::kLast, Buffers{}.geom(geom, geom_bytes, binned || geom).binning(binning, binning_bytes).image(image, image_bytes, !fwd_only))) return rc;
    if (c.blend.forward == ForwardBlend::kDevicePicked) if (int rc = check_present(kGeom, geom)) return rc;
    if (int rc = bin_duplicates(c, D)) return rc;
    {
        StageTimer t(SR_STAGE_BLEND_FWD, c.s);
        SR_HIP(launch_render_forward(c.f, c.B.ranges, c.B.order, c.B.point_list, binned ? c.G.recs : nullptr, g->colors_precomp, out_color, out_allmap,
                                     c.I.final_T, c.I.n_contrib, fwd_only ? nullptr : c.B.hit_mask, c.blend,
                                     reinterpret_cast<unsigned long long*>(frame->blend_counters), c.G.counts, c.s));
    }
    return debug_sync(frame, c.s, "render_forward");
}

size_t sr_class_image_bytes(int32_t W, int32_t H, int32_t n_classes) { return class_layout(W, H, n_classes).total; }

int sr_class_forward_render(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                            size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t D, float* out_dist, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kClassPass, false, stream, ClassPass{n_classes, ClassIds::kInColors, false})) return rc;
    if (!binning || !class_image || !out_dist) return fail(SR_ERR_INVALID_ARGUMENT, "binning / class_image / out_dist is NULL");
    if (c.P > 0 && !geom) return fail(SR_ERR_INVALID_ARGUMENT, "geom is NULL (the class ids of the P Gaussians are staged in it, even when no duplicate was emitted)");
    if (int rc = c.bind(D, GeomOrder::kLast, Buffers{}.geom(geom, geom_bytes, c.P > 0).binning(binning, binning_bytes).cls(class_image, class_image_bytes))) return rc;
    const FrameDev& f = c.f; const BinView& B = c.B; const ClassView& C = c.C; hipStream_t s = c.s;
    if (int rc = bin_duplicates(c, D)) return rc;
    {
        // every tile list, stably partitioned by class: [class 0 by depth | class 1 by depth | ...] + a (begin, end) pair per (tile, class)
        StageTimer t(SR_STAGE_CLASS_PARTITION, s);
        uint8_t* ids = reinterpret_cast<uint8_t*>(c.G.sh_jac);   // (nullptr where P == 0: no geometry buffer was bound)
        SR_HIP(launch_class_partition(c.P, f.tiles_x * f.tiles_y, n_classes, g->colors_precomp, nullptr, B.ranges, B.point_list, ids, B.class_list(), C.ranges, s));
    }
    if (int rc = debug_sync(frame, s, "class_partition")) return rc;
    {
        StageTimer t(SR_STAGE_CLASS_FWD, s);
        SR_HIP(launch_class_forward(f, n_classes, C.ranges, B.order, B.class_list(), c.P > 0 && D > 0 ? c.G.recs : nullptr, out_dist, C.state, C.last, C.tile_total, B.hit_mask,
                                    (frame->flags & SR_FLAG_NO_QUADRANT_CULL) ? 0 : 1, s));
    }
    return debug_sync(frame, s, "class_forward");
}

int sr_class_backward(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* radii, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* class_image, size_t class_image_bytes, uint32_t D, const float* dL_ddist,
                      void* workspace, size_t workspace_bytes, const SrGradients* grads, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kClassPass, true, stream, ClassPass{n_classes, ClassIds::kInColors, false})) return rc;
    if (!grads) return fail(SR_ERR_INVALID_ARGUMENT, "grads is NULL");
    const int P = c.P;
    if (P == 0) return SR_OK;
    if (!radii || !dL_ddist) return fail(SR_ERR_INVALID_ARGUMENT, "radii / dL_ddist is NULL");
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).binning(binning, binning_bytes).cls(class_image, class_image_bytes).workspace(workspace, workspace_bytes, 3))) return rc;
    const FrameDev& f = c.f; const GeomView& G = c.G; const BinView& B = c.B; const ClassView& C = c.C; const WorkspaceView& ws = c.ws; hipStream_t s = c.s;
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
size_t sr_class_shared_bytes(int32_t P, int32_t W, int32_t H, int32_t n_classes, uint32_t D) { return class_shared_layout(P, W, H, n_classes, D).total; }

int sr_class_forward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, const int32_t* classes, void* geom, size_t geom_bytes,
                            void* binning, size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t D, float* out_dist, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kClassPass, false, stream, ClassPass{n_classes, ClassIds::kOwnArray, true})) return rc;
    const int P = c.P;
    if (!binning || !class_state || !out_dist || (P > 0 && !classes)) return fail(SR_ERR_INVALID_ARGUMENT, "binning / class_state / out_dist / classes is NULL");
    // (the geometry buffer: for the records alone, so only where something was binned)
    if (int rc = c.bind(D, GeomOrder::kLast, Buffers{}.geom(geom, geom_bytes, P > 0 && D > 0).binning(binning, binning_bytes).cls(class_state, class_state_bytes))) return rc;
    const FrameDev& f = c.f; const BinView& B = c.B; const ClassView& C = c.C; hipStream_t s = c.s;
    {
        StageTimer t(SR_STAGE_CLASS_PARTITION, s);
        SR_HIP(launch_class_partition(P, f.tiles_x * f.tiles_y, n_classes, nullptr, classes, B.ranges, B.point_list, C.ids, B.class_list(), C.ranges, s));
    }
    if (int rc = debug_sync(frame, s, "class_partition")) return rc;
    {
        StageTimer t(SR_STAGE_CLASS_FWD, s);
        SR_HIP(launch_class_forward(f, n_classes, C.ranges, B.order, B.class_list(), c.G.recs, out_dist, C.state, C.last, C.tile_total, C.hit,
                                    (frame->flags & SR_FLAG_NO_QUADRANT_CULL) ? 0 : 1, s));
    }
    return debug_sync(frame, s, "class_forward");
}

int sr_class_backward_shared(const SrFrame* frame, const SrGaussians* g, int32_t n_classes, void* geom, size_t geom_bytes, void* binning,
                             size_t binning_bytes, void* class_state, size_t class_state_bytes, uint32_t D, const float* dL_ddist, void* workspace,
                             size_t workspace_bytes, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kClassPass, true, stream, ClassPass{n_classes, ClassIds::kOwnArray, false})) return rc;
    if (c.P == 0 || D == 0) return SR_OK;
    if (!dL_ddist) return fail(SR_ERR_INVALID_ARGUMENT, "dL_ddist is NULL");
    // (the workspace: the records and flags sr_backward_blend of the SAME frame left in it -- this pass adds to them)
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).binning(binning, binning_bytes).cls(class_state, class_state_bytes)
                                                       .workspace(workspace, workspace_bytes, g->color_channels))) return rc;
    const BinView& B = c.B; const ClassView& C = c.C;
    {
        StageTimer t(SR_STAGE_CLASS_BWD, c.s);
        SR_HIP(launch_class_backward(c.f, n_classes, C.ranges, B.order, B.class_list(), c.G.recs, C.state, C.last, C.tile_total, dL_ddist, C.hit,
                                     c.ws.records, c.ws.written, (int)(record_bytes(g->color_channels) / 16), c.s));
    }
    return debug_sync(frame, c.s, "class_backward_shared");
}

int sr_backward_blend(const SrFrame* frame, const SrGaussians* g, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                      void* image, size_t image_bytes, uint32_t D, const float* dL_dcolor, const float* dL_dallmap, void* workspace,
                      size_t workspace_bytes, void* stream) {
    Call c{};
    if (int rc = c.open(frame, g, Checks::kBlend, true, stream)) return rc;
    if (c.P == 0) return SR_OK;
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).binning(binning, binning_bytes).image(image, image_bytes)
                                                       .workspace(workspace, workspace_bytes, g->color_channels))) return rc;
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
    Call c{};
    if (int rc = c.open(frame, g, Checks::kCommon, true, stream)) return rc;
    if (c.P == 0) return SR_OK;
    if (g->color_channels == 6 || g->color_channels == 9) return fail(SR_ERR_UNSUPPORTED, "sr_backward_colors serves the 3-channel pass");
    if (!radii || !dL_dcolors) return fail(SR_ERR_INVALID_ARGUMENT, "radii / dL_dcolors is NULL");
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).workspace(workspace, workspace_bytes, g->color_channels))) return rc;
    StageTimer t(SR_STAGE_PREPROCESS_BWD, c.s);
    SR_HIP(launch_color_gradients(c.P, c.f, radii, c.G.clamped, c.G.recs, c.ws.records, c.ws.written, c.G.tiles_touched, g->shs != nullptr, dL_dcolors, c.s));
    return debug_sync(frame, c.s, "color_gradients");
}

int sr_backward_geometry(const SrFrame* frame, const SrGaussians* g, const int32_t* radii, void* geom, size_t geom_bytes,
                         void* binning, size_t binning_bytes, void* image, size_t image_bytes, uint32_t D, void* workspace,
                         size_t workspace_bytes, const SrGradients* grads, void* stream) {
    if (!grads) return fail(SR_ERR_INVALID_ARGUMENT, "grads is NULL");
    Call c{};
    if (int rc = c.open(frame, g, Checks::kBlend, true, stream)) return rc;
    if (c.P == 0) return SR_OK;
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).binning(binning, binning_bytes).image(image, image_bytes)
                                                       .workspace(workspace, workspace_bytes, g->color_channels))) return rc;
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
    Call c{};
    if (int rc = c.open(frame, g, Checks::kCommon, false, stream)) return rc;
    if (c.P == 0 || D == 0) return SR_OK;
    if (!valid_bits || !use3d_bits) return fail(SR_ERR_INVALID_ARGUMENT, "valid_bits / use3d_bits is NULL");
    if (int rc = c.bind(D, GeomOrder::kFirst, Buffers{}.geom(geom, geom_bytes).binning(binning, binning_bytes))) return rc;
    SR_HIP(launch_pair_decisions(c.f, c.B.ranges, c.B.point_list, c.G.recs,
                                 reinterpret_cast<unsigned long long*>(valid_bits), reinterpret_cast<unsigned long long*>(use3d_bits), c.s));
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

int sr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                    void* stream) {
    (void)projmatrix;
    if (P < 0) return fail(SR_ERR_INVALID_ARGUMENT, "P < 0");
    if (P == 0) return SR_OK;
    if (!means3D || !viewmatrix || !present) return fail(SR_ERR_INVALID_ARGUMENT, "NULL argument");
    SR_HIP(launch_mark_visible(P, means3D, viewmatrix, present, static_cast<hipStream_t>(stream)));
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
