// blend_common.h -- device helpers shared by the blend kernels (render.hip: K6 / decision dump, render_bwd.hip: K7; render_class.hip: the
// per-class distortion pass): staging of list entries into the tile-local form, exact quadrant culling, the ray-splat test,
// the emission index of a duplicate, the wave-level transpose-reduction of the per-entry gradient sums, the hit-mask encoding and its
// decoder, the forward's per-pixel state / step / stores (ForwardPixel ...) and the backward's per-pair arithmetic (BackwardPixel ...).
#pragma once
#include "common.h"
#include "footprint_cull.h"   // fast_rcp, the quadrant / cell culling of the staging lane (also compiled on the host by its test)

namespace sr {

constexpr int kWave = 64;
constexpr int kXcds = 8;   // MI355X: 8 accelerator dies, workgroup i runs on XCD i % 8
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kFN = kFar / (kFar - kNear);

// s_waitcnt vmcnt(0) (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima), placed by hand at the
// top of a round of the list walks: everything in flight there was issued a round earlier, and a wait that sits on EVERY control-flow
// path lets the compiler's own counter tracking start the round from zero -- a wait inside the (lane < n) staging branch leaves the
// skip path "pending", and the next use of a prefetched register then waits again, behind whatever store was issued in between.
__device__ __forceinline__ void wait_vector_memory() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// counters of the K6 counter variant (SrFrame.blend_counters, caller-owned, 16 x u64): [0] entries staged, [1] entries with a
// non-zero quadrant mask, [2] quadrant tests executed, [3] quadrant tests with >= 1 valid lane, [4] valid (pixel, entry) pairs,
// [5] / [6] tests with a valid pixel in rows 0-3 / rows 4-7 of the quadrant, [7] entries with a valid pixel anywhere in the tile,
// [8] (entry, 4x4 cell) pairs with a valid pixel, [9] sum over (round of 64 entries, quadrant) of the busiest cell's pair count,
// [10] / [11] the same two with the pairs the row-mapped forward's cell culling at staging KEEPS (hits and misses) instead of the exact hits
// (cell_mask_rows: slab extents since the octagon-vs-cell test left; the benchmark still prints them under the octagon's name),
// [12] / [13] unused, zero (an octagon + oriented-box culling, measured and removed: DESIGN.md 4), [14] exact (entry, cell) pairs that
// the staging test of [10] would DROP (must be 0), [15] the pairs of [10] as the octagon-vs-cell test would keep them

// (counter variant only) the sixteen 4x4 cells of a 16x16 tile, bit 4 q + c = cell c of quadrant q, cell c at (c & 1, c >> 1) inside its
// quadrant: bits 0..15 by the test the row-mapped forward stages with (cell_mask_rows: slab extents), bits 16..31 by the octagon test it
// replaced -- the yardstick of slot [15].
__device__ __forceinline__ uint32_t cell_mask16(const float Tu[3], const float Tv[3], const float Tw[3], float mx, float my, float opacity) {
    return cell_mask_rows<2, 2>(Tu, Tv, Tw, mx, my, opacity, 0.f) | (cell_mask_octagon<2, 2>(Tu, Tv, Tw, mx, my, opacity, 0.f) << 16);
}

// ---------------------------------------------------------------------------------------------
// Staged entry layout in LDS (struct-of-quads, s_e[quad][slot]):
//   e0 = A.xyz B.x | e1 = B.yz C.xy | e2 = C.z Tw.xyz | e3 = xy'.x xy'.y opacity c5
//   e4 = n.xyz c0  | e5 = c1 c2 c3 c4  | (9 channels only) e6 = c6 c7 c8 -
// with A = Tv' x Tw, B = Tw x Tu', C = Tu' x Tv' and ' = relative to the tile centre (Xc, Yc); c0..c2 = rgb.  SURVEY 8f N1:
// NC = 6 blends six precomputed channels (the two 3-channel one-hot passes of render_semantic as ONE pass), NC = 9 blends the
// SH colour AND six precomputed channels (render + render_semantic as one pass).  Channels 3.. come straight from the caller's
// [P,6] array at staging time: columns 3..5 for NC = 6 (columns 0..2 went through K1 into the record), all six for NC = 9.
// ---------------------------------------------------------------------------------------------
template <int NC> constexpr int entry_quads() { return NC == 9 ? 7 : (NC == 0 ? 4 : 6); }   // NC = 0: geometry only (e0..e3: the per-class distortion pass)

__device__ __forceinline__ float4 load_extra(const float* __restrict__ colors6, uint32_t gid, int first) {
    const float* c = colors6 + 6 * (size_t)gid + first;
    return make_float4(c[0], c[1], c[2], 0.f);
}

template <int QX, int QY, int NC>
__device__ __forceinline__ uint32_t stage_entry(const float4 (&q)[kRecQuads], const float4 ex, const float4 ey, float Xc, float Yc, int cull,
                                                float4 (*s_e)[kWave], int slot, float yshift = 0.f, uint32_t* cells16 = nullptr, uint32_t* cells_rows = nullptr,
                                                bool slab_cells = true) {
    const float Tw[3] = {q[1].z, q[1].w, q[2].x};
    const float Tu[3] = {q[0].x - Xc * Tw[0], q[0].y - Xc * Tw[1], q[0].z - Xc * Tw[2]};
    const float Tv[3] = {q[0].w - Yc * Tw[0], q[1].x - Yc * Tw[1], q[1].y - Yc * Tw[2]};
    const float A[3] = {Tv[1] * Tw[2] - Tv[2] * Tw[1], Tv[2] * Tw[0] - Tv[0] * Tw[2], Tv[0] * Tw[1] - Tv[1] * Tw[0]};
    const float B[3] = {Tw[1] * Tu[2] - Tw[2] * Tu[1], Tw[2] * Tu[0] - Tw[0] * Tu[2], Tw[0] * Tu[1] - Tw[1] * Tu[0]};
    const float C[3] = {Tu[1] * Tv[2] - Tu[2] * Tv[1], Tu[2] * Tv[0] - Tu[0] * Tv[2], Tu[0] * Tv[1] - Tu[1] * Tv[0]};
    const float mx = q[2].y - Xc, my = q[2].z - Yc, opacity = q[2].w;
    s_e[0][slot] = make_float4(A[0], A[1], A[2], B[0]);
    s_e[1][slot] = make_float4(B[1], B[2], C[0], C[1]);
    s_e[2][slot] = make_float4(C[2], Tw[0], Tw[1], Tw[2]);
    // p.z = x A.z + y B.z + C.z vanishes at EVERY pixel when a scale (or the quaternion) is exactly zero -- the three coefficients are then
    // exact zeros, here as in the reference's cross(k, l), whose `if (p.z == 0) continue` drops such a splat altogether: it is staged
    // with opacity 0 and never passes the alpha test.  (An isolated p.z == 0 of a healthy splat is rounding noise: see intersect().)
    const bool plane_degenerate = A[2] == 0.f && B[2] == 0.f && C[2] == 0.f;
    s_e[3][slot] = make_float4(mx, my, plane_degenerate ? 0.f : opacity, ex.z);
    if (NC != 0) {
        s_e[4][slot] = make_float4(q[3].x, q[3].y, q[3].z, q[3].w);   // n.xyz, c0  (component-wise: a whole-quad copy of an array element keeps the array in scratch)
        s_e[5][slot] = make_float4(q[4].x, q[4].y, ex.x, ex.y);   // c1, c2 | c3, c4
    }
    if (NC == 9) s_e[6][slot] = make_float4(ey.x, ey.y, ey.z, 0.f);
    if (cells16) *cells16 = cell_mask16(Tu, Tv, Tw, mx, my, opacity);   // (counter variant: what a 4x4-cell culling would keep)
    if (cells_rows) {   // (row-mapped forward: per-cell bits; a quadrant is visited if one of its cells is)
        // slab_cells = false: the octagon test -- the forward that writes cell-granular hit masks spills at its 80 registers with the slab extents
        *cells_rows = slab_cells ? cell_mask_rows<QX, QY>(Tu, Tv, Tw, mx, my, opacity, yshift) : cell_mask_octagon<QX, QY>(Tu, Tv, Tw, mx, my, opacity, yshift);
        uint32_t qm = 0;
#pragma unroll
        for (int q = 0; q < QX * QY; ++q) qm |= ((*cells_rows >> (4 * q)) & 15u) ? (1u << q) : 0u;
        return qm;
    }
    return cull ? quadrant_mask<QX, QY>(Tu, Tv, Tw, mx, my, opacity, yshift) : (1u << (QX * QY)) - 1u;
}

struct Hit {
    float sx, sy, dx, dy, depth, G, alpha, pz_inv;
    bool use3d;
};

// Ray-splat intersection + alpha at tile-local pixel (xl, yl); branch-free, returns the validity predicate
// (the chain of `continue`s of Appendix A.4, with the same comparison senses so NaNs behave alike).
__device__ __forceinline__ bool intersect(float xl, float yl, const float4 e0, const float4 e1, const float4 e2, const float4 e3,
                                          Hit& h) {
    const float ppx = fmaf(xl, e0.x, fmaf(yl, e0.w, e1.z));
    const float ppy = fmaf(xl, e0.y, fmaf(yl, e1.x, e1.w));
    const float ppz = fmaf(xl, e0.z, fmaf(yl, e1.y, e2.x));
    h.pz_inv = fast_rcp(ppz);
    h.sx = ppx * h.pz_inv; h.sy = ppy * h.pz_inv;
    const float rho3d = h.sx * h.sx + h.sy * h.sy;
    h.dx = e3.x - xl; h.dy = e3.y - yl;
    const float rho2d = kFilterInvSquare * (h.dx * h.dx + h.dy * h.dy);
    const bool use2d = !(rho3d <= rho2d);   // (ONE compare serves the depth select here and the path branch of the backward)
    h.use3d = !use2d;
    const float rho = fminf(rho3d, rho2d);
    h.depth = use2d ? e2.w : fmaf(h.sx, e2.y, fmaf(h.sy, e2.z, e2.w));
    h.G = __builtin_amdgcn_exp2f(rho * (-0.5f * kLog2e));   // exp(-rho / 2)
    h.alpha = fminf(kAlphaCap, e3.z * h.G);
    // (the reference also skips on `power > 0`: never true -- rho3d and rho2d are sums of squares, fminf drops a NaN operand, and a NaN
    // power fails that test as well -- so the comparison is not evaluated here)
    // The reference's `if (p.z == 0) continue` (Appendix A.4; SR_REFERENCE_PZ_SKIP = 1, the shipped value) is evaluated on the staged cross
    // product p.z = x A.z + y B.z + C.z.  For a healthy splat p.z == 0 means the pixel's ray is parallel to the splat's plane: a set of
    // measure zero in exact arithmetic, and in float32 a coin toss among the pairs whose p.z is pure rounding noise -- which of them land on
    // exactly 0 depends on the operation order, so this expression and the reference's cross(k, l).z can skip DIFFERENT pairs of that
    // noise set (the oracle's margin walk classifies them; profiles/r05_parity_c3.json counts them).  A splat whose p.z vanishes
    // identically (a zero scale) has three exact-zero coefficients and is skipped everywhere, here as there.
    // SR_REFERENCE_PZ_SKIP = 0 (variant pz_zero_through_filter) is the exact-arithmetic rule instead: with ppz = 0, rcp gives inf, rho3d is
    // inf or NaN, the comparison above takes the screen-space path and fminf drops rho3d -- the pair is blended through its 2-D filter
    // footprint, what exact arithmetic does with the astronomically large rho3d of a nearly parallel ray (identically-zero splats are
    // dropped at staging: stage_entry).  sx, sy, pz_inv are only read on the ray-splat path.
#if SR_REFERENCE_PZ_SKIP
    return !(h.depth < kNear) & !(h.alpha < kAlphaFloor) & !(ppz == 0.f);   // upstream's per-pair `if (p.z == 0) continue`, on THIS cross product
#else
    return !(h.depth < kNear) & !(h.alpha < kAlphaFloor);
#endif
}

// Emission index of the duplicate (tile tx,ty ; Gaussian gid): duplicates are emitted per Gaussian, y-major /
// x-minor over its tile rectangle (same expressions as K1 / K3 -> same rectangle).
__device__ __forceinline__ uint32_t emission_index(const float4 (&q)[kRecQuads], uint32_t first, int tx, int ty, const FrameDev& f) {
    const float cx = q[2].y, cy = q[2].z, radius = q[4].w;
    int minx = (int)((cx - radius) * f.inv_tile_w), miny = (int)((cy - radius) * f.inv_tile_h);
    int maxx = (int)((cx + radius + (float)(f.tile_w - 1)) * f.inv_tile_w);
    minx = min(f.tiles_x, max(0, minx)); maxx = min(f.tiles_x, max(0, maxx));
    miny = min(f.tiles_y, max(0, miny));
    return first + (uint32_t)((ty - miny) * (maxx - minx) + (tx - minx));
}

// the 18 floats the forward blend stages (everything but depth and radius): four dwordx4 + one dwordx2
__device__ __forceinline__ void load_record18(const float4* __restrict__ recs, uint32_t gid, float4 (&q)[kRecQuads]) {
    const float4* r = recs + (size_t)gid * kRecQuads;
#pragma unroll
    for (int k = 0; k < kRecQuads - 1; ++k) q[k] = r[k];
    const float2 t = *reinterpret_cast<const float2*>(r + (kRecQuads - 1));
    q[kRecQuads - 1].x = t.x; q[kRecQuads - 1].y = t.y;
}
__device__ __forceinline__ void load_record(const float4* __restrict__ recs, uint32_t gid, float4 (&q)[kRecQuads]) {
    const float4* r = recs + (size_t)gid * kRecQuads;
#pragma unroll
    for (int k = 0; k < kRecQuads; ++k) q[k] = r[k];
}
// the three record quads the class pass stages (transform rows, centre, opacity); the others keep what they hold
__device__ __forceinline__ void load_record_geometry(const float4* __restrict__ recs, uint32_t gid, float4 (&q)[kRecQuads]) {
    const float4* r = recs + (size_t)gid * kRecQuads;
    q[0] = r[0]; q[1] = r[1]; q[2] = r[2];
}


// ---------------------------------------------------------------------------------------------
// wave-level transpose-reduction of 24 values per lane (gfx950):
//   fold across the two 32-lane halves with v_permlane32_swap (value k <-> k+12), across row pairs with
//   v_permlane16_swap (k <-> k+6), then a 4-step DPP row rotation sum.  60 VALU ops for 24 values (a plain
//   butterfly needs 144 cross-lane ops).  Afterwards every lane of 16-lane row g holds, in v[0..5], the
//   64-lane totals of values 6g .. 6g+5.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void fold32(float& a, float& b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ void fold16(float& a, float& b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int kCtrl>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xf, 0xf, false));
}
// value of lane ^ 4, without the LDS crossbar: a row rotation by 12 (= left by 4) into the lanes whose bit 2 is clear (DPP
// banks 0 and 2) and by 4 into the others (banks 1 and 3); row_ror:n delivers lane (l - n) mod 16
__device__ __forceinline__ float dpp_xor4(float x) {
    int t = __builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x12C, 0xf, 0x5, false);
    t = __builtin_amdgcn_update_dpp(t, __float_as_int(x), 0x124, 0xf, 0xA, false);
    return __int_as_float(t);
}
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp_mov<0x128>(x);  // row_ror:8
    x += dpp_mov<0x124>(x);  // row_ror:4
    x += dpp_mov<0x122>(x);  // row_ror:2
    x += dpp_mov<0x121>(x);  // row_ror:1
    return x;
}
// Returns the 64-lane totals of the 24 values, one per lane: lane l ends up with the total of value index
//   reduce24_index(l) = (bit1(l) ? 2 : bit4(l)) + 3 bit5(l) + 6 bit2(l) + 12 bit3(l),
// valid in the lanes with bit0 clear and not (bit1 and bit4) -- 24 lanes.
// DPP first: the two in-row levels (lane ^ 8, lane ^ 4) are transposing folds done with bank-masked DPP adds -- the rotated operand
// rides in the add itself (1.8 ns per wave instruction against 3.9 + 1.05 for a lane swap plus its add), two instructions per pair
// of registers and no selects: the first writes the banks that keep `a`, the second the banks that keep `b`.  24 -> 12 -> 6 registers
// cost 36 DPP adds; only then do the cross-row levels run on 6 registers (5 swaps instead of 18), and the quad levels on 2.
// Measured against the swap-first order it replaces (18 swaps + 9 DPP moves + 27 adds + 14 selects): tools/ubench/reduce_ubench.hip.
// One asm block: the DPP reads of a register follow its last write by >= 7 instructions inside the block (the hardware wants 2
// wait states between a VALU write and a DPP read, and the compiler's hazard recogniser does not look into inline asm); the
// s_nop in front covers whatever wrote the inputs.
// NV = 24, or 21: values 21..23 are not in use (three colour channels) -- they need no reset and no fold; their slots of the result hold
// copies of other totals, which nothing reads.
// Preconditions: ALL 64 lanes active (DPP without bound_ctrl leaves the destination of a lane whose source is disabled untouched: the
// callers run the fold outside any divergent region -- K7's entry loop is wave-uniform); the twelve outputs are early-clobber ("+&v"):
// they are overwritten while the input-only registers are still to be read, so no input may share a register with an output.
template <int NV>
__device__ __forceinline__ void dpp_fold_rows(float (&v)[24]) {
    static_assert(NV == 24 || NV == 21, "24 values, or 21 with the last three unused");
    if (NV == 24) {
        asm volatile(
        "s_nop 1\n"
        // level lane^8, lanes 0-7 of every row: v[k] += v[k] of lane^8 (all lanes written; lanes 8-15 are overwritten next)
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %5, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %7, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %8, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %9, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %10, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %11, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        // ... lanes 8-15 (banks 2, 3) take value k + 12 instead
        "v_add_f32_dpp %0, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %1, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %2, %14, %14 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %3, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %4, %16, %16 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %5, %17, %17 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %6, %18, %18 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %7, %19, %19 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %8, %20, %20 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %9, %21, %21 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %10, %22, %22 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %11, %23, %23 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        // level lane^4: lanes with bit 2 clear (banks 0, 2) keep register k (partner = lane + 4: row_ror:12), lanes with bit 2 set
        // (banks 1, 3) take register k + 6 (partner = lane - 4: row_ror:4)
        "v_add_f32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %4, %4, %4 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %5, %5, %5 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %0, %6, %6 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %1, %7, %7 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %2, %8, %8 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %3, %9, %9 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %4, %10, %10 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %5, %11, %11 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "s_nop 1\n"
        : "+&v"(v[0]), "+&v"(v[1]), "+&v"(v[2]), "+&v"(v[3]), "+&v"(v[4]), "+&v"(v[5]), "+&v"(v[6]), "+&v"(v[7]), "+&v"(v[8]), "+&v"(v[9]), "+&v"(v[10]), "+&v"(v[11])
        : "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]), "v"(v[16]), "v"(v[17]), "v"(v[18]), "v"(v[19]), "v"(v[20]), "v"(v[21]), "v"(v[22]), "v"(v[23]));
    } else {
        asm volatile(
        "s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %5, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %7, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %8, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %9, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %10, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %11, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %0, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %1, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %2, %14, %14 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %3, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %4, %16, %16 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %5, %17, %17 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %6, %18, %18 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %7, %19, %19 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %8, %20, %20 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %4, %4, %4 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %5, %5, %5 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %0, %6, %6 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %1, %7, %7 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %2, %8, %8 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %3, %9, %9 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %4, %10, %10 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %5, %11, %11 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "s_nop 1\n"
        : "+&v"(v[0]), "+&v"(v[1]), "+&v"(v[2]), "+&v"(v[3]), "+&v"(v[4]), "+&v"(v[5]), "+&v"(v[6]), "+&v"(v[7]), "+&v"(v[8]), "+&v"(v[9]), "+&v"(v[10]), "+&v"(v[11])
        : "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]), "v"(v[16]), "v"(v[17]), "v"(v[18]), "v"(v[19]), "v"(v[20]));
    }
}
// ---------------------------------------------------------------------------------------------
// Zeros from the LDS (round 6).  The backward kernels clear 15..24 accumulator registers per list entry; as v_mov instructions that was 8 % of K7's
// vector instructions.  The same registers filled by broadcast ds_read_b128 of a small block of zeros cost the vector unit nothing: the loads issue
// down the LDS port -- which these kernels leave three-quarters idle -- beside the entry's own four, and the compiler's counter tracking lets the
// ray-splat test start while they are in flight.  Four copies of the block, picked by the entry slot: an address that changes per entry keeps the
// loads inside the entry loop (a loop-invariant address would be hoisted and the zeros copied with -- v_mov).  The block is written through an
// opaque register, so its contents are not a constant the loads could be folded into.  C3: K7 1.670 -> 1.615 ms, bit-identical (same-box A/B).
// ---------------------------------------------------------------------------------------------
constexpr int kZeroCopies = 4;
template <int kQuads>
__device__ __forceinline__ void lds_zeros_init(float4 (*s_zero)[kZeroCopies], int lane) {   // by every lane of (one of) the workgroup's waves; same-wave readers need no barrier
    float zo = 0.f;
    asm volatile("" : "+v"(zo));
    if (lane < kQuads * kZeroCopies) s_zero[lane / kZeroCopies][lane % kZeroCopies] = make_float4(zo, zo, zo, zo);
}
template <int kN, int kLen>
__device__ __forceinline__ void lds_zeros_load(const float4 (*s_zero)[kZeroCopies], int slot, float (&v)[kLen]) {   // v[0 .. kN) from the LDS, the rest plain zeros
    const int zi = slot & (kZeroCopies - 1);
#pragma unroll
    for (int k = 0; k < (kN + 3) / 4; ++k) {
        const float4 z = s_zero[k][zi];
        if (4 * k < kN) v[4 * k] = z.x;
        if (4 * k + 1 < kN) v[4 * k + 1] = z.y;
        if (4 * k + 2 < kN) v[4 * k + 2] = z.z;
        if (4 * k + 3 < kN) v[4 * k + 3] = z.w;
    }
#pragma unroll
    for (int k = kN; k < kLen; ++k) v[k] = 0.f;
}

// LDS float add without a return value (ds_add_f32): one wave's adds to an address land in program order
__device__ __forceinline__ void lds_add_f32(float* p, float x) { (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int reduce24_index(int l) { return ((l & 2) ? 2 : ((l >> 4) & 1)) + 3 * ((l >> 5) & 1) + 6 * ((l >> 2) & 1) + 12 * ((l >> 3) & 1); }
__device__ __forceinline__ bool reduce24_holds_total(int l) { return (l & 1) == 0 && !((l & 2) && (l & 16)); }
template <int NV = 24>
__device__ __forceinline__ float wave_reduce24(float (&v)[24], int lane) {
    dpp_fold_rows<NV>(v);                          // v[0..5]: value k + 6 bit2 + 12 bit3, summed over the lanes {l, l^4, l^8, l^12}
#pragma unroll
    for (int k = 0; k < 3; ++k) fold32(v[k], v[k + 3]);    // + 3 bit5, summed over both halves
    float z = 0.f;
    fold16(v[0], v[1]);                        // bit4 clear: value 0 (+ ...), bit4 set: value 1; summed over all four rows
    fold16(v[2], z);                           // bit4 clear: value 2; bit4 set: nothing
    float a = v[0], b = v[2];
    // the two quad levels as four DPP adds (written out: left to the compiler the last level became v_mov 0 + v_mov_dpp + v_add per value, the add
    // sunk into the caller's `holds_total` branch); the s_nops are the two wait states between a vector write and its DPP read
    asm volatile(
        "s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"   // lane ^ 2
        "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
        "s_nop 0\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"   // lane ^ 1: every lane of a quad holds the totals
        "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
        : "+v"(a), "+v"(b));
    return (lane & 2) ? b : a;
}

// The same reduction for 16 values (the per-class distortion backward: 15 live accumulators): 16 -> 8 -> 4 registers in-row (24 bank-masked
// DPP adds), two half folds and one row-pair fold on 4 registers (3 swaps), two quad levels on one.  26 DPP + 3 swaps against the 40 + 5
// of wave_reduce24.  Afterwards EVERY lane holds the 64-lane total of value reduce16_index(lane); the lanes with bits 0 and 1 clear
// (16 of them) cover all sixteen.  Same preconditions as dpp_fold_rows (all 64 lanes active; >= 7 instructions between a write and
// its DPP read inside the block: 8 here).
__device__ __forceinline__ int reduce16_index(int l) { return ((l >> 4) & 1) + 2 * ((l >> 5) & 1) + 4 * ((l >> 2) & 1) + 8 * ((l >> 3) & 1); }
__device__ __forceinline__ bool reduce16_holds_total(int l) { return (l & 3) == 0; }
__device__ __forceinline__ float wave_reduce16(float (&v)[16]) {
    asm volatile(
        "s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %5, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %7, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xf\n"
        "v_add_f32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %1, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %2, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %4, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %5, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %6, %14, %14 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %7, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc\n"
        "v_add_f32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %2, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %3, %3, %3 row_ror:12 row_mask:0xf bank_mask:0x5\n"
        "v_add_f32_dpp %0, %4, %4 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %1, %5, %5 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %2, %6, %6 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "v_add_f32_dpp %3, %7, %7 row_ror:4 row_mask:0xf bank_mask:0xa\n"
        "s_nop 1\n"
        : "+&v"(v[0]), "+&v"(v[1]), "+&v"(v[2]), "+&v"(v[3]), "+&v"(v[4]), "+&v"(v[5]), "+&v"(v[6]), "+&v"(v[7])
        : "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]));
    fold32(v[0], v[2]); fold32(v[1], v[3]);   // lanes < 32: values 0 / 1 (+ 4 bit2 + 8 bit3), lanes >= 32: values 2 / 3
    fold16(v[0], v[1]);                       // bit4 clear: value 0 or 2, bit4 set: value 1 or 3; summed over all four rows
    float a = v[0];
    asm volatile(   // (written out as in wave_reduce24)
        "s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"   // lane ^ 2
        "s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"   // lane ^ 1
        : "+v"(a));
    return a;
}

// 64-lane totals of three more values (the 9-channel variant): afterwards every lane of 16-lane row r holds the total of value r
// (row 3: zero).  Two half folds, one row-pair fold, one in-row sum.
__device__ __forceinline__ float wave_reduce3(float a, float b, float c) {
    float d = 0.f;
    fold32(a, b); fold32(c, d);   // a: lanes < 32 hold a's half sums, lanes >= 32 b's;  c: c's | zeros
    fold16(a, c);                 // rows 0..3: a, c, b, zero
    return row_sum16(a);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, m));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// Exact (entry, quadrant) hit mask for the backward: K7 visits only the pairs that reached a pixel in the forward.  16 bits per list entry;
// two-band tiles (16x16, 32x16): low byte = the QX quadrant bits of the upper band, high byte = those of the lower band.
template <int QX, int QY, int SPLIT>
__device__ __forceinline__ void store_hit_mask(uint16_t* __restrict__ hit_mask, uint32_t pos, int part, uint32_t hm) {
    if (SPLIT == 2) reinterpret_cast<uint8_t*>(hit_mask)[2 * (size_t)pos + part] = (uint8_t)hm;
    else if (QY == 2) hit_mask[pos] = (uint16_t)((hm & ((1u << QX) - 1u)) | ((hm >> QX) << 8));
    else hit_mask[pos] = (uint16_t)hm;
}
template <int QX, int QY>
__device__ __forceinline__ uint32_t decode_hits(uint16_t h) {
    return QY == 2 ? (((uint32_t)h & ((1u << QX) - 1u)) | ((((uint32_t)h >> 8) & ((1u << QX) - 1u)) << QX)) : (uint32_t)h;
}
// a round's hits wait as scalar ballots (bit j of hit[q] = entry j reached a pixel of quadrant q): the quadrant bits of the entry `lane` stages
template <int NQ>
__device__ __forceinline__ uint32_t lane_hit_bits(const unsigned long long (&hit)[NQ], int lane) {
    uint32_t hm = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) hm |= (uint32_t)((hit[q] >> lane) & 1ull) << q;
    return hm;
}

// ---------------------------------------------------------------------------------------------
// The blend forward's straight-line pieces, written once: which band of which tile a workgroup owns, a pixel's running state, its step for
// a pair that passed `intersect`, and its stores.  The walks (staging pipeline, prefetch distances, ballot / row loops, barriers) differ
// for measured reasons and stay in the kernels (render.hip, render_class.hip).  Everything here is inlined into its callers.
// ---------------------------------------------------------------------------------------------
// A binning tile (QX*8 wide, QY*8*SPLIT high) is walked by SPLIT band waves.  Workgroups are dealt round-robin to the 8 XCDs, each with its
// own L2: the SPLIT bands of one tile take consecutive slots of the SAME XCD, so that the second band finds the tile's records in that L2
// instead of fetching them again (the grid is rounded up to whole XCD rows, so a slot can lie past the last tile: the caller returns).
// (Xc, Yc): the local origin = centre of the binning tile, shared with K7 (identical staged values, identical decisions); yshift_px: this
// band's quadrants relative to that centre.  Two steps, the caller's `return` between them: with the test inside, the origin's arithmetic
// was scheduled in front of the branch.
struct Band { int tile, part, tx0, ty0, yshift_px; float Xc, Yc; };
template <int SPLIT>
__device__ __forceinline__ void band_of_block(Band& b) {   // -> b.tile (still the slot in tile_order), b.part
    b.tile = blockIdx.x; b.part = 0;
    if (SPLIT > 1) {
        const int xcd = blockIdx.x % kXcds, k = blockIdx.x / kXcds;
        b.tile = (k / SPLIT) * kXcds + xcd; b.part = k % SPLIT;
    }
}
template <int QX, int QY, int SPLIT>
__device__ __forceinline__ void band_origin(const FrameDev& f, const uint32_t* tile_order, Band& b) {
    b.tile = (int)tile_order[b.tile];   // longest lists first (binning.hip tile_order_kernel)
    b.tx0 = (b.tile % f.tiles_x) * (QX * 8); b.ty0 = (b.tile / f.tiles_x) * (QY * 8 * SPLIT) + b.part * (QY * 8);
    b.Xc = (float)(b.tx0 + QX * 4); b.Yc = (float)((b.tile / f.tiles_x) * (QY * 8 * SPLIT) + QY * SPLIT * 4);
    b.yshift_px = b.part * (QY * 8) - QY * (SPLIT - 1) * 4;
}

// T > 0: the pixel is live.  T < 0: done (saturated, or outside the image) -- |T| is its final transmittance.  (A separate flag per pixel
// costs a byte compare, two moves and a four-instruction all-done test per quadrant test.)  C3..C8 are only live with 6 / 9 channels.
struct ForwardPixel {
    float T, C0, C1, C2, N0, N1, N2, Dsum, M1, M2, dist, med, C3, C4, C5, C6, C7, C8;
    uint32_t lastc, medc;   // last / median contributor (1-based list position)
};
__device__ __forceinline__ void init_forward_pixel(ForwardPixel& p, bool inside) {
    p.T = inside ? 1.f : -1.f; p.C0 = p.C1 = p.C2 = p.N0 = p.N1 = p.N2 = 0.f;
    p.C3 = p.C4 = p.C5 = p.C6 = p.C7 = p.C8 = 0.f;
    p.Dsum = p.M1 = p.M2 = p.dist = p.med = 0.f;
    p.lastc = 0; p.medc = 0xFFFFFFFFu;
}
// the distortion sums of a blended pair (T: the transmittance in front of it, w = alpha T); shared with the per-class distortion pass
__device__ __forceinline__ void distortion_step(float& dist, float& M1, float& M2, float T, float depth, float w) {
    const float A = 1.f - T;
    const float mm = kFN * (1.f - kNear * fast_rcp(depth));
    dist += (mm * mm * A + M2 - 2.f * mm * M1) * w;
    M1 += mm * w;
    M2 += mm * mm * w;
}
// One live pixel and one entry that passed `intersect`.  e3..e6: the staged entry (e6: colour channels 6..8, read with NC = 9 only; by value,
// the others by reference: the one combination that leaves the register counts of every instantiation where they were).
template <int NC>
__device__ __forceinline__ void blend_forward_step(ForwardPixel& p, const Hit& h, const float4& e3, const float4& e4, const float4& e5, const float4 e6, uint32_t contributor) {
    const float test_T = p.T * (1.f - h.alpha);
    const bool go = !(test_T < kTStop);   // else: done, and this entry is NOT blended
    if (go) {
        const float w = h.alpha * p.T;
        p.Dsum += h.depth * w;
        distortion_step(p.dist, p.M1, p.M2, p.T, h.depth, w);
        if (p.T > 0.5f) { p.med = h.depth; p.medc = contributor; }
        p.N0 += e4.x * w; p.N1 += e4.y * w; p.N2 += e4.z * w;
        p.C0 += e4.w * w; p.C1 += e5.x * w; p.C2 += e5.y * w;
        if (NC >= 6) { p.C3 += e5.z * w; p.C4 += e5.w * w; p.C5 += e3.w * w; }
        if (NC == 9) { p.C6 += e6.x * w; p.C7 += e6.y * w; p.C8 += e6.z * w; }
        p.lastc = contributor;
    }
    p.T = go ? test_T : -p.T;
}
// The pixel's outputs (channel order: DESIGN.md) and, final_T != NULL, the backward's per-pixel state (NULL with SR_FLAG_FORWARD_ONLY).
template <int NC>
__device__ __forceinline__ void store_forward_pixel(const ForwardPixel& p, const FrameDev& f, const float3 bg, size_t pix, float* __restrict__ out_color, float* __restrict__ out_allmap,
                                                    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib) {
    const size_t HW = (size_t)f.H * f.W;
    const float Tq = fabsf(p.T);
    if (final_T) {
        final_T[pix] = Tq; final_T[HW + pix] = p.M1; final_T[2 * HW + pix] = p.M2;
        n_contrib[pix] = p.lastc; n_contrib[HW + pix] = p.medc;
    }
    out_color[pix] = p.C0 + Tq * bg.x;
    out_color[HW + pix] = p.C1 + Tq * bg.y;
    out_color[2 * HW + pix] = p.C2 + Tq * bg.z;
    if (NC >= 6) {
        out_color[3 * HW + pix] = p.C3 + Tq * f.bg[3];
        out_color[4 * HW + pix] = p.C4 + Tq * f.bg[4];
        out_color[5 * HW + pix] = p.C5 + Tq * f.bg[5];
    }
    if (NC == 9) {
        out_color[6 * HW + pix] = p.C6 + Tq * f.bg[6];
        out_color[7 * HW + pix] = p.C7 + Tq * f.bg[7];
        out_color[8 * HW + pix] = p.C8 + Tq * f.bg[8];
    }
    out_allmap[pix] = p.Dsum;
    out_allmap[HW + pix] = 1.f - Tq;
    out_allmap[2 * HW + pix] = p.N0; out_allmap[3 * HW + pix] = p.N1; out_allmap[4 * HW + pix] = p.N2;
    out_allmap[5 * HW + pix] = p.med;
    out_allmap[6 * HW + pix] = p.dist;
}

// ---------------------------------------------------------------------------------------------
// The blend backward, written once: what the three K7 kernels (render_bwd.hip: one wave per tile, cooperative, row-mapped) and the
// per-class distortion backward (render_class.hip) have in common.  Everything here is inlined into its callers.
// ---------------------------------------------------------------------------------------------
// A per-entry sum takes its term by accumulation (several pixels of a lane add into registers that start from zeros) or, kAccumulate =
// false, by assignment (the cooperative K7: one pixel per lane, so there is nothing to add to -- an accumulate into its LDS-loaded zeros
// would cost the VALU-bound kernel ~21 vector instructions per pair, and `0 + x` is not `x` in the sign of a zero).
template <bool kAccumulate> __device__ __forceinline__ void sum_term(float& s, float x) { s = kAccumulate ? s + x : x; }
template <bool kAccumulate> __device__ __forceinline__ void sum_term(float& s, float a, float b) { s = kAccumulate ? fmaf(a, b, s) : a * b; }

// The geometry sums of one (pixel, entry) pair, v[0..13]: on the ray-splat path the moments of dL/dp in tile-local pixel coordinates
// (shifted to the Gaussian's own centre when the record is written: moment_shift; the cross products happen once per Gaussian in K8),
// on the screen-space filter path dL/d(means2D).  (xq, yq): the pixel, tile-local; Twx, Twy: the staged e2.y, e2.z.
template <bool kAccumulate, bool kFuseSx, int kLen>
__device__ __forceinline__ void geometry_sums(const Hit& h, float xq, float yq, float Twx, float Twy, float dL_dG, float dL_dz, float (&v)[kLen]) {
    if (h.use3d) {
        const float gG = -dL_dG * h.G;
        // gG s + dL_dz Tw is ONE fma and one rounded product.  Written as a plain sum, contraction fuses whichever product the optimiser
        // leaves on the left, and that differed from instantiation to instantiation; kFuseSx pins what each kernel has always computed
        // (true: the sx / sy product is the fused one) -- the gradients differ in the last bit between the two.
        const float tx = kFuseSx ? fmaf(gG, h.sx, dL_dz * Twx) : fmaf(dL_dz, Twx, gG * h.sx);
        const float ty = kFuseSx ? fmaf(gG, h.sy, dL_dz * Twy) : fmaf(dL_dz, Twy, gG * h.sy);
        const float dpx = tx * h.pz_inv, dpy = ty * h.pz_inv;
        const float dpz = -(dpx * h.sx + dpy * h.sy);
        sum_term<kAccumulate>(v[0], dpx); sum_term<kAccumulate>(v[1], dpy); sum_term<kAccumulate>(v[2], dpz);
        sum_term<kAccumulate>(v[3], xq, dpx); sum_term<kAccumulate>(v[4], xq, dpy); sum_term<kAccumulate>(v[5], xq, dpz);
        sum_term<kAccumulate>(v[6], yq, dpx); sum_term<kAccumulate>(v[7], yq, dpy); sum_term<kAccumulate>(v[8], yq, dpz);
        sum_term<kAccumulate>(v[9], dL_dz, h.sx); sum_term<kAccumulate>(v[10], dL_dz, h.sy);
    } else {
        const float gG = -dL_dG * h.G * kFilterInvSquare;
        sum_term<kAccumulate>(v[12], gG, h.dx);
        sum_term<kAccumulate>(v[13], gG, h.dy);
    }
    sum_term<kAccumulate>(v[11], dL_dz);   // (both paths)
}

// One pixel of K7: the upstream gradients folded with the forward's final accumulators, and the state of the back-to-front walk.
struct BackwardPixel {
    float gr, gg, gb, gn0, gn1, gn2, g_depth, g_median, a0, a1, a2;
    float gc[6];             // upstream gradients of colour channels 3..8 (6- / 9-channel variants)
    uint32_t lastc, medc;    // last / median contributor of the forward
    float T, Z;              // transmittance in front of the entry the walk is at; the suffix sum (render.hip)
};
template <int NC>
__device__ __forceinline__ void load_backward_pixel(const FrameDev& f, int px, int py, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                                                    const float* __restrict__ dL_dcolor, const float* __restrict__ dL_dallmap, BackwardPixel& p) {
    const size_t HW = (size_t)f.H * f.W;
    const bool inside = px < f.W && py < f.H;
    const size_t pix = inside ? (size_t)py * f.W + px : 0;
    const float T_final = inside ? final_T[pix] : 0.f;
    const float fin_D = inside ? final_T[HW + pix] : 0.f, fin_D2 = inside ? final_T[2 * HW + pix] : 0.f;
    p.lastc = inside ? n_contrib[pix] : 0u;
    p.medc = inside ? n_contrib[HW + pix] : 0u;
    p.gr = inside ? dL_dcolor[pix] : 0.f; p.gg = inside ? dL_dcolor[HW + pix] : 0.f; p.gb = inside ? dL_dcolor[2 * HW + pix] : 0.f;
    p.g_depth = inside ? dL_dallmap[pix] : 0.f;
    const float g_accum = inside ? dL_dallmap[HW + pix] : 0.f;
    p.gn0 = inside ? dL_dallmap[2 * HW + pix] : 0.f; p.gn1 = inside ? dL_dallmap[3 * HW + pix] : 0.f; p.gn2 = inside ? dL_dallmap[4 * HW + pix] : 0.f;
    p.g_median = inside ? dL_dallmap[5 * HW + pix] : 0.f;
    const float g_reg = inside ? dL_dallmap[6 * HW + pix] : 0.f;
    float bg_dot = f.bg[0] * p.gr + f.bg[1] * p.gg + f.bg[2] * p.gb;
    p.gc[0] = p.gc[1] = p.gc[2] = p.gc[3] = p.gc[4] = p.gc[5] = 0.f;
    if (NC >= 6) {
        p.gc[0] = inside ? dL_dcolor[3 * HW + pix] : 0.f; p.gc[1] = inside ? dL_dcolor[4 * HW + pix] : 0.f; p.gc[2] = inside ? dL_dcolor[5 * HW + pix] : 0.f;
        bg_dot += f.bg[3] * p.gc[0] + f.bg[4] * p.gc[1] + f.bg[5] * p.gc[2];
    }
    if (NC == 9) {
        p.gc[3] = inside ? dL_dcolor[6 * HW + pix] : 0.f; p.gc[4] = inside ? dL_dcolor[7 * HW + pix] : 0.f; p.gc[5] = inside ? dL_dcolor[8 * HW + pix] : 0.f;
        bg_dot += f.bg[6] * p.gc[3] + f.bg[7] * p.gc[4] + f.bg[8] * p.gc[5];
    }
    p.a0 = (1.f - T_final) * g_reg; p.a1 = fin_D * g_reg; p.a2 = fin_D2 * g_reg;
    p.T = T_final; p.Z = -T_final * (g_accum - bg_dot);   // the background / alpha term rides in the suffix sum
}

// The per-pair arithmetic of K7 for a pair that passed `intersect`: steps the pixel's T and Z, adds the pair's terms to the entry's sums
// v[0..23] and returns the blend weight w (the 9-channel kernel forms three more sums from it).  e2..e6: the staged entry (e6: colour
// channels 6..8, read with NC = 9 only).
//   psi = rgb.g + depth g_depth + n.gn + (a2 + m (m a0 - 2 a1)), m = the depth metric; dL/dz = w (2 (m a0 - a1) dm/dz + g_depth),
//   dm/dz = kFN kNear / depth^2.  t1 = m a0 - a1 serves both: 8 instructions where the literal transcription took 11.  (The three
//   distortion terms cancel to the variance of m along the ray: they are combined in ONE fma before anything else is added -- seeding
//   the colour chain with a2 saves another instruction and costs a digit under a distortion-weighted loss.)
// kXG = false: the sums of dL/dcolors_precomp are not formed (render_bwd.hip).  kFuseSx: see geometry_sums.
template <int NC, bool kXG, bool kAccumulate, bool kFuseSx>
__device__ __forceinline__ float blend_backward_pair(const float4 e2, const float4 e3, const float4 e4, const float4 e5, const float4 e6, const Hit& h,
                                                     float xq, float yq, uint32_t cidx, BackwardPixel& p, float (&v)[24]) {
    const float one_m_inv = fast_rcp(1.f - h.alpha);
    p.T *= one_m_inv;                 // transmittance in front of this entry
    const float w = h.alpha * p.T;
    float phi = fmaf(e4.w, p.gr, fmaf(e5.x, p.gg, fmaf(e5.y, p.gb, fmaf(h.depth, p.g_depth,
                fmaf(e4.x, p.gn0, fmaf(e4.y, p.gn1, e4.z * p.gn2))))));
    if (NC >= 6) phi = fmaf(e5.z, p.gc[0], fmaf(e5.w, p.gc[1], fmaf(e3.w, p.gc[2], phi)));
    if (NC == 9) phi = fmaf(e6.x, p.gc[3], fmaf(e6.y, p.gc[4], fmaf(e6.z, p.gc[5], phi)));
    const float inv_depth = fast_rcp(h.depth);
    const float m_d = fmaf(inv_depth, -kFN * kNear, kFN);
    const float t1 = fmaf(m_d, p.a0, -p.a1);
#if SR_DETACH_WEIGHT
    const float psi = phi;   // upstream DETACH_WEIGHT: the distortion does not differentiate through the blend weights
#else
    const float psi = phi + fmaf(m_d, t1 - p.a1, p.a2);
#endif
    const float dL_dalpha = p.T * psi - one_m_inv * p.Z;
    p.Z = fmaf(w, psi, p.Z);
    const float med_add = (cidx == p.medc - (SR_MEDIAN_CONTRIBUTOR_MINUS_ONE ? 1u : 0u)) ? p.g_median : 0.f;
    const float dL_dz = fmaf(w, fmaf(t1 * (inv_depth * inv_depth), 2.f * kFN * kNear, p.g_depth), med_add);
    const float dL_dG = e3.z * dL_dalpha;
    if (NC != 6 || kXG) { sum_term<kAccumulate>(v[18], w * p.gr); sum_term<kAccumulate>(v[19], w * p.gg); sum_term<kAccumulate>(v[20], w * p.gb); }   // (6 channels: all of them precomputed)
    if (NC >= 6 && kXG) { sum_term<kAccumulate>(v[21], w * p.gc[0]); sum_term<kAccumulate>(v[22], w * p.gc[1]); sum_term<kAccumulate>(v[23], w * p.gc[2]); }
    sum_term<kAccumulate>(v[15], w * p.gn0); sum_term<kAccumulate>(v[16], w * p.gn1); sum_term<kAccumulate>(v[17], w * p.gn2);
    sum_term<kAccumulate>(v[14], h.G * dL_dalpha);
    geometry_sums<kAccumulate, kFuseSx>(h, xq, yq, e2.y, e2.z, dL_dG, dL_dz, v);
    return w;
}

// The shift of the moments Sx, Sy from tile-local coordinates to coordinates relative to the Gaussian's OWN centre (cx, cy): sum (xl - mx) dp
// = sum xl dp - mx S0 with mx = cx - Xc.  K8 sums these over the Gaussian's tiles and works with Tu - cx Tw, Tv - cy Tw: the same dL/dT as
// with moments about the image origin, without the cancellation of pixel coordinates ~1000 against extents of a few pixels (clamped into the
// image: the moments of a splat whose centre projects far off-screen are taken about the nearest image point).
__device__ __forceinline__ void moment_shift(const float4 (&q)[kRecQuads], float Xc, float Yc, const FrameDev& f, float& ox, float& oy) {
    const float mx = q[2].y - Xc, my = q[2].z - Yc;   // (the staged centre: same expression, same bits as stage_entry's)
    ox = -fminf(fmaxf(mx, -Xc), (float)(f.W - 1) - Xc); oy = -fminf(fmaxf(my, -Yc), (float)(f.H - 1) - Yc);
}
// Clears the lane's row of s_out for the round that begins; kShiftInLds: the shift waits for the flush in slots 22, 23 of the row
template <int kGQ, bool kShiftInLds>
__device__ __forceinline__ void reset_record_row(float* row, float ox, float oy) {
    float4* z = reinterpret_cast<float4*>(row);
#pragma unroll
    for (int k = 0; k < kGQ; ++k) z[k] = (kShiftInLds && k == 5) ? make_float4(0.f, 0.f, ox, oy) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The memory pipeline of the backward walk.  Nothing that comes back from memory is touched in the round that asks for it:
//   * the list entry (gid) of round r - 2 is requested during round r, the record of round r - 1 (address = that gid, which arrived a
//     round ago) too, RAW -- first[] and first_base[] stay two registers and the hit mask stays undecoded until round r - 1 stages them;
//   * the records of round r are STORED at the top of round r - 1, behind its staging and behind this prefetch: the wave's vector-memory
//     counter retires in issue order, so the wait at the top of the round (wait_vector_memory, on every path) has the same number of
//     younger memory operations behind the last load on every path: none.
// A dependent `gid = list[pos]; record(gid); first[gid] + first_base[..]` inside the round made the wave wait for two memory round trips
// (and for the stores of the previous flush in front of them) in EVERY round: SQ_WAIT_INST_ANY was 26 % of the wave cycles
// (profiles/r05_c3_sq_counters.json).
// NC: the colour channels of the caller (6 / 9: channels 3.. come from `extra`, see stage_entry); 0 = geometry only (the class pass: the
// three geometry quads and the radius word that emission_index reads).  `idx`: the entry of a round this lane stages.
template <int NC>
struct WalkPrefetch {
    float4 nr[kRecQuads], nx = make_float4(0.f, 0.f, 0.f, 0.f), ny = nx;   // the record; colour channels 3.. (NC = 6 / 9)
    uint32_t nfirst = 0, nfbase = 0, nhraw = 0, gid_ahead = 0;
    __device__ __forceinline__ void fetch(const FrameDev& f, const float4* __restrict__ recs, const float* __restrict__ extra, const uint16_t* __restrict__ hit_mask,
                                          uint32_t gid, uint32_t pos) {
        if (NC == 0) {
            load_record_geometry(recs, gid, nr);
            nr[4].w = reinterpret_cast<const float*>(recs + (size_t)gid * kRecQuads + 4)[3];
        } else {
            load_record(recs, gid, nr);
        }
        nfirst = f.first[gid]; nfbase = f.first_base[gid / kScanTile];
        if (NC == 6) nx = load_extra(extra, gid, 3);
        if (NC == 9) { nx = load_extra(extra, gid, 0); ny = load_extra(extra, gid, 3); }
        nhraw = hit_mask[pos];
    }
    // before the walk: the deepest round's record, the list entry of the round in front of it (every round but the last one is full);
    // stages: this lane stages entries at all (the cooperative K7: sixteen lanes per wave)
    __device__ __forceinline__ void begin(const FrameDev& f, const float4* __restrict__ recs, const float* __restrict__ extra, const uint16_t* __restrict__ hit_mask,
                                          const uint32_t* __restrict__ list, uint32_t list_begin, int rounds, uint32_t total, int idx, bool stages = true) {
        if (NC == 0) {   // (geometry only: the quads fetch() does not load are zeros)
#pragma unroll
            for (int i = 0; i < kRecQuads; ++i) nr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (stages && rounds > 0 && (uint32_t)((rounds - 1) * kWave + idx) < total) {
            const uint32_t pos = list_begin + (rounds - 1) * kWave + idx;
            fetch(f, recs, extra, hit_mask, list[pos], pos);
        }
        if (stages && rounds > 1) gid_ahead = list[list_begin + (rounds - 2) * kWave + idx];
    }
    // in round rd (entries rbase ..), behind its staging and in front of its flush
    __device__ __forceinline__ void advance(const FrameDev& f, const float4* __restrict__ recs, const float* __restrict__ extra, const uint16_t* __restrict__ hit_mask,
                                            const uint32_t* __restrict__ list, uint32_t list_begin, int rd, uint32_t rbase, int idx) {
        if (rd > 0) {   // (the next round is always full)
            fetch(f, recs, extra, hit_mask, gid_ahead, list_begin + rbase - kWave + idx);
            if (rd > 1) gid_ahead = list[list_begin + rbase - 2 * kWave + idx];
        }
    }
};

// Tile shapes (BASELINE config 5's sweep): the reference's 16x16 plus 8x8, 16x8, 32x8, 32x16 = QX x QY quadrants of 8x8
// pixels, i.e. 1 / 2 / 4 / 8 pixels per lane.  (In a launcher: `f` is its FrameDev, an unknown shape returns from it.)
#define SR_FOR_TILE_SHAPE(F)                                                    \
    if (f.tile_w == 16 && f.tile_h == 16) { F(2, 2); }                          \
    else if (f.tile_w == 8 && f.tile_h == 8) { F(1, 1); }                       \
    else if (f.tile_w == 16 && f.tile_h == 8) { F(2, 1); }                      \
    else if (f.tile_w == 32 && f.tile_h == 8) { F(4, 1); }                      \
    else if (f.tile_w == 32 && f.tile_h == 16) { F(4, 2); }                     \
    else return hipErrorInvalidValue;


}  // namespace sr
