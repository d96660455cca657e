// footprint_cull.h -- the staging lane's culling geometry: which quadrants / 4x4 cells of a tile an entry's alpha >= 1/255 footprint can
// reach.  Included by blend_common.h for the kernels; free of HIP types, so that tests/cell_cull_host.cpp compiles the SAME routines with
// the system compiler and holds them to `intersect`'s acceptance rule pixel by pixel (host build: sqrtf / logf / 1.f / x behind the wrappers).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SR_CULL_FN __device__ __forceinline__
#else
#include <math.h>
#define SR_CULL_FN inline
#endif

namespace sr {

#if defined(__HIPCC__)
SR_CULL_FN float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
SR_CULL_FN float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
SR_CULL_FN float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
SR_CULL_FN float fast_log(float x) { return __logf(x); }
#else
SR_CULL_FN float fast_rcp(float x) { return 1.f / x; }
SR_CULL_FN float fast_sqrt(float x) { return sqrtf(x); }
SR_CULL_FN float fast_rsq(float x) { return 1.f / sqrtf(x); }
SR_CULL_FN float fast_log(float x) { return logf(x); }
#endif

// ---------------------------------------------------------------------------------------------
// Quadrant culling.  A list entry can only contribute to a pixel if alpha = min(0.99, opacity*G) >= 1/255,
// i.e. rho = min(rho3d, rho2d) <= thr = 2 ln(255 opacity).  {rho3d <= thr} is the image of the disc
// u^2+v^2 <= thr under the splat's homography -- an ellipse with dual conic C* = Q diag(thr,thr,-1) Q^T --
// and {rho2d <= thr} is a disc of radius sqrt(thr/2) around means2D.  The staging lane bounds that union by
// an octagon (support in directions x, y, x+y, x-y from the tangent-line equation l^T C* l = 0) and tests it
// against the tile's 8x8 quadrants (QX x QY of them; 2 x 2 for the reference's 16x16 tile).  (A second, nearly exact test in the splat's (u,v) plane removes another
// 9 % of the tests but costs more at staging than it saves -- measured, not kept.)  Entries dropped here are entries the per-pixel test would skip anyway (`continue` in Appendix A.4),
// so results are unchanged; the bound has 0.3 px / 1 % slack for float rounding and keeps the entry whenever
// anything is degenerate or NaN.  Inputs are tile-local (origin at
// the tile centre), which keeps the conic free of cancellation.
// ---------------------------------------------------------------------------------------------
// The footprint's dual conic, formed once for the octagon and for the slab extents.  det = thr * det(Tu; Tv; Tw): det C* = -det^2.
struct FootprintConic { float thr, c00, c01, c11, c02, c12, c22, det; };
// Returns 0 = empty footprint, 2 = unbounded (the cutoff disc reaches the camera plane, or something is degenerate: keep the entry
// everywhere), 1 = a bounded ellipse.
SR_CULL_FN int footprint_conic(const float Tu[3], const float Tv[3], const float Tw[3], float opacity, FootprintConic& k) {
    float thr = 2.f * fast_log(255.f * opacity);
    thr = thr * 1.01f + 0.01f;
    k.thr = thr;
    if (thr <= 0.f) return 0;
    k.c22 = thr * (Tw[0] * Tw[0] + Tw[1] * Tw[1]) - Tw[2] * Tw[2];
    if (!(k.c22 < 0.f)) return 2;  // the cutoff disc reaches the camera plane: unbounded footprint
    k.c00 = thr * (Tu[0] * Tu[0] + Tu[1] * Tu[1]) - Tu[2] * Tu[2];
    k.c01 = thr * (Tu[0] * Tv[0] + Tu[1] * Tv[1]) - Tu[2] * Tv[2];
    k.c11 = thr * (Tv[0] * Tv[0] + Tv[1] * Tv[1]) - Tv[2] * Tv[2];
    k.c02 = thr * (Tu[0] * Tw[0] + Tu[1] * Tw[1]) - Tu[2] * Tw[2];
    k.c12 = thr * (Tv[0] * Tw[0] + Tv[1] * Tw[1]) - Tv[2] * Tw[2];
    k.det = thr * (Tu[0] * (Tv[1] * Tw[2] - Tv[2] * Tw[1]) + Tu[1] * (Tv[2] * Tw[0] - Tv[0] * Tw[2]) + Tu[2] * (Tv[0] * Tw[1] - Tv[1] * Tw[0]));
    return 1;
}
// octagon of the entry's footprint in tile-local coordinates: lo / hi of x, y, x + y, x - y (of a bounded conic: footprint_conic == 1)
SR_CULL_FN void octagon_bounds(const FootprintConic& k, float mx, float my, float (&lo)[4], float (&hi)[4]) {
    const float c22 = k.c22;
    const float inv = fast_rcp(c22);
    const float r = fast_sqrt(0.5f * k.thr);
    const float QA[4] = {k.c00, k.c11, k.c00 + 2.f * k.c01 + k.c11, k.c00 - 2.f * k.c01 + k.c11};
    const float QB[4] = {k.c02, k.c12, k.c02 + k.c12, k.c02 - k.c12};
    const float ctr[4] = {mx, my, mx + my, mx - my};
    const float rad[4] = {r, r, r * 1.4142137f, r * 1.4142137f};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int d = 0; d < 4; ++d) {
        const float disc = QB[d] * QB[d] - QA[d] * c22;
        const float half = fast_sqrt(fmaxf(disc, 0.f)) * (-inv) * 1.01f;
        const float dc = QB[d] * inv;
        lo[d] = fminf(dc - half, ctr[d] - rad[d]);
        hi[d] = fmaxf(dc + half, ctr[d] + rad[d]);
    }
}
// ... from the staged rows.  Returns footprint_conic's kind; lo / hi are valid for kind 1.
SR_CULL_FN int octagon_bounds(const float Tu[3], const float Tv[3], const float Tw[3], float mx, float my, float opacity,
                              float (&lo)[4], float (&hi)[4]) {
    FootprintConic k;
    const int kind = footprint_conic(Tu, Tv, Tw, opacity, k);
    if (kind == 1) octagon_bounds(k, mx, my, lo, hi);
    return kind;
}
// does the octagon reach the pixel-centre rectangle [x0, x1] x [y0, y1] (0.3 px of slack for float rounding)?
SR_CULL_FN bool octagon_reaches(const float (&lo)[4], const float (&hi)[4], float x0, float x1, float y0, float y1) {
    const float m = 0.3f;
    x0 -= m; y0 -= m; x1 += m; y1 += m;
    return !(lo[0] > x1 || hi[0] < x0 || lo[1] > y1 || hi[1] < y0 || lo[2] > x1 + y1 || hi[2] < x0 + y0 || lo[3] > x1 - y0 || hi[3] < x0 - y1);
}

template <int QX, int QY>
SR_CULL_FN uint32_t quadrant_mask(const float Tu[3], const float Tv[3], const float Tw[3], float mx, float my,
                                  float opacity, float yshift) {
    constexpr uint32_t kAll = (1u << (QX * QY)) - 1u;
    float lo[4], hi[4];
    const int kind = octagon_bounds(Tu, Tv, Tw, mx, my, opacity, lo, hi);
    if (kind != 1) return kind ? kAll : 0u;
    // the wave's quadrants sit `yshift` below the local origin: shift the bounds instead of the (compile-time) rectangles
    lo[1] -= yshift; hi[1] -= yshift; lo[2] -= yshift; hi[2] -= yshift; lo[3] += yshift; hi[3] += yshift;
    uint32_t mask = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < QX * QY; ++q) {   // quadrant (q % QX, q / QX) of the tile, coordinates relative to the tile centre
        const float x0 = (float)((q % QX) * 8 - QX * 4), y0 = (float)((q / QX) * 8 - QY * 4);
        if (octagon_reaches(lo, hi, x0, x0 + 7.f, y0, y0 + 7.f)) mask |= 1u << q;
    }
    return mask;
}
// The octagon against the four 4x4 cells of each of the wave's quadrants: bit 4 q + c = cell c of quadrant q, cell c at (c & 1, c >> 1)
// inside its quadrant.  What the row-mapped forward staged with before the slab extents below; kept as the yardstick of the counter
// variant (slot [15]) and of tests/cell_cull_host.cpp.
template <int QX, int QY>
SR_CULL_FN uint32_t cell_mask_octagon(const float Tu[3], const float Tv[3], const float Tw[3], float mx, float my,
                                      float opacity, float yshift) {
    constexpr uint32_t kAll = (QX * QY >= 8) ? 0xFFFFFFFFu : (1u << (4 * QX * QY)) - 1u;
    float lo[4], hi[4];
    const int kind = octagon_bounds(Tu, Tv, Tw, mx, my, opacity, lo, hi);
    if (kind != 1) return kind ? kAll : 0u;
    lo[1] -= yshift; hi[1] -= yshift; lo[2] -= yshift; hi[2] -= yshift; lo[3] += yshift; hi[3] += yshift;
    uint32_t mask = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < QX * QY; ++q)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < 4; ++c) {
            const float x0 = (float)((q % QX) * 8 + (c & 1) * 4 - QX * 4), y0 = (float)((q / QX) * 8 + (c >> 1) * 4 - QY * 4);
            if (!octagon_reaches(lo, hi, x0, x0 + 3.f, y0, y0 + 3.f)) continue;
            mask |= 1u << (4 * q + c);
        }
    return mask;
}

// ---------------------------------------------------------------------------------------------
// Slab extents: the footprint's exact x interval inside a horizontal slab of pixel rows.  The ellipse {rho3d <= thr} is convex, so its
// part inside the slab ya <= y <= yb is convex and projects onto x as ONE interval; a cell of that row of cells can hold a footprint pixel
// only if its x range meets the interval -- exact for the geometry where the octagon of a slanted, elongated splat is loose.
// With centre c = (c02, c12) / c22 and shape S = (c0 c0^T - c22 C*_2x2) / c22^2 the ellipse is (X - c)^T S^-1 (X - c) <= 1, and its chord
// on the line y = t, dy = t - cy, is
//     x = cx + (sxy / syy) dy  +-  sqrt(K (1 - dy^2 / syy)),     K = det S / syy,    det S = det C* / c22^3 = -det^2 / c22^3
// (det S from the determinant of the staged rows, not as sxx syy - sxy^2, which cancels for a thin slanted splat).  The right end of the
// chord is concave in t with its maximum at the ellipse's rightmost point, y = cy + sxy / sqrt(sxx), so over the slab it is largest on
// the line nearest to that point: t = clamp(cy + sxy / sqrt(sxx), ya, yb); the left end likewise with cy - sxy / sqrt(sxx).  Two chord
// ends per slab give the exact extent -- they ARE the chords on the two boundary lines and the extreme points where those lie inside; the
// chord through the centre's y lies between them and adds nothing.  The filter disc {rho2d <= thr} adds mx +- sqrt(r^2 - dy^2), dy =
// distance of my from the slab; the two intervals are joined.
// Slack as in the octagon test: thr * 1.01 + 0.01; the ellipse grown by 1 % about its centre (S * 1.01^2: half-widths, and the y range
// the chords are cut from -- what absorbs the rounding of a footprint thousands of pixels wide, whose 1 - dy^2 / syy cancels); 0.3 px on
// every bound (the caller's ya / yb carry theirs).  S also gets + (0.1 px)^2 on its diagonal -- a superset, at most 0.1 px wider -- so
// that a needle whose sxx or syy is rounding noise still has a slope and a K with a meaning.  A NaN anywhere keeps the whole row of
// cells (the clamps and the `< 0` guards below are written so that a NaN passes through them, unlike fminf / fmaxf).
// ---------------------------------------------------------------------------------------------
struct SlabExtent { float cx, cy, syy, isyy, slope, K, ytop, mx, my, r2; bool finite; };   // ytop = sxy / sqrt(sxx): y of the rightmost point - cy
SR_CULL_FN void slab_extent_setup(const FootprintConic& k, float mx, float my, SlabExtent& s) {
    const float kGrow = 1.0201f, kPad = 0.01f;
    const float inv = fast_rcp(k.c22), inv2 = inv * inv * kGrow;
    s.cx = k.c02 * inv; s.cy = k.c12 * inv;
    const float sxx0 = (k.c02 * k.c02 - k.c00 * k.c22) * inv2, sxy = (k.c02 * k.c12 - k.c01 * k.c22) * inv2;
    const float syy0 = (k.c12 * k.c12 - k.c11 * k.c22) * inv2;
    const float det0 = -(k.det * k.det) * (inv2 * inv2) * k.c22;   // det (1.01^2 S) = -det^2 1.01^4 / c22^3
    const float sxx = sxx0 + kPad;
    s.syy = syy0 + kPad;
    s.isyy = fast_rcp(s.syy);
    s.slope = sxy * s.isyy;
    s.K = (det0 + kPad * (sxx0 + s.syy)) * s.isyy;   // det (S + pad I) = det S + pad (sxx + syy) + pad^2
    s.ytop = sxy * fast_rsq(sxx);
    s.mx = mx; s.my = my; s.r2 = 0.5f * k.thr;
    // an inf or a NaN in any row, in the centre or in the opacity reaches one of these (cx: Tu, cy: Tv, all: Tw and thr); the blend's own
    // test lets a NaN pair through at every pixel, so such an entry must keep every cell
    const float t = fabsf(s.cx) + fabsf(s.cy) + fabsf(s.slope) + fabsf(s.K) + fabsf(s.ytop) + fabsf(s.syy) + fabsf(mx) + fabsf(my);
    s.finite = t < 3.0e38f;
}
// x interval [lo, hi] of the footprint inside ya <= y <= yb, 0.3 px of slack included; lo > hi: nothing of it lies in the slab
SR_CULL_FN void slab_interval(const SlabExtent& s, float ya, float yb, float& lo, float& hi) {
    const float kNone = 3.0e38f, m = 0.3f;
    // ellipse: its y range is cy +- sqrt(syy)
    float de = ya - s.cy;                      // distance of the centre from the slab (<= 0 inside), NaN-preserving
    de = (s.cy - yb > de) ? s.cy - yb : de;
    float tr = s.cy + s.ytop, tl = s.cy - s.ytop;
    tr = tr < ya ? ya : tr; tr = tr > yb ? yb : tr;
    tl = tl < ya ? ya : tl; tl = tl > yb ? yb : tl;
    const float dr = tr - s.cy, dl = tl - s.cy;
    float wr = s.K - s.K * s.isyy * dr * dr, wl = s.K - s.K * s.isyy * dl * dl;
    wr = wr < 0.f ? 0.f : wr; wl = wl < 0.f ? 0.f : wl;
    float er = s.cx + s.slope * dr + fast_sqrt(wr) + m, el = s.cx + s.slope * dl - fast_sqrt(wl) - m;
    const bool e_none = de > 0.f && de * de > s.syy;
    er = e_none ? -kNone : er; el = e_none ? kNone : el;
    // filter disc
    float dd = ya - s.my;
    dd = (s.my - yb > dd) ? s.my - yb : dd;
    dd = dd < 0.f ? 0.f : dd;
    const float h2 = s.r2 - dd * dd;
    const float h = fast_sqrt(h2 < 0.f ? 0.f : h2);
    const float fr = h2 < 0.f ? -kNone : s.mx + h + m, fl = h2 < 0.f ? kNone : s.mx - h - m;
    const float chk = (el + er) + (fl + fr);   // NaN if any of the four is (an empty interval's ends cancel)
    lo = fminf(el, fl); hi = fmaxf(er, fr);
    if (!(chk == chk)) { lo = -kNone; hi = kNone; }
}

// The cells of the wave's quadrants (bit layout of cell_mask_octagon) by slab extents: one interval per row of cells -- a band of QY
// quadrant rows has 2 QY slabs of four pixel rows, its cells have the x ranges [x0, x0 + 3] -- instead of four octagon tests per row.
// Exact where the octagon is loose -- a slanted, elongated splat; the pair and step counts at C3 are in DESIGN.md 4.  (Two more slabs along the principal axes of the footprint ellipse, an oriented box on top of the octagon, kept 6 % fewer pairs than
// the octagon alone and cost as much at staging as they saved: measured, not kept -- DESIGN.md 4.)
template <int QX, int QY>
SR_CULL_FN uint32_t cell_mask_rows(const float Tu[3], const float Tv[3], const float Tw[3], float mx, float my,
                                   float opacity, float yshift) {
    constexpr uint32_t kAll = (QX * QY >= 8) ? 0xFFFFFFFFu : (1u << (4 * QX * QY)) - 1u;
    FootprintConic k;
    const int kind = footprint_conic(Tu, Tv, Tw, opacity, k);
    if (kind != 1) return kind ? kAll : 0u;
    SlabExtent s;
    slab_extent_setup(k, mx, my, s);
    if (!s.finite) return kAll;
    s.cy -= yshift; s.my -= yshift;   // the wave's quadrants sit `yshift` below the local origin
    uint32_t mask = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 2 * QY; ++r) {   // row r of cells: cell row r & 1 of quadrant row r >> 1
        const float y0 = (float)(r * 4 - QY * 4);
        float lo, hi;
        slab_interval(s, y0 - 0.3f, y0 + 3.3f, lo, hi);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 2 * QX; ++i) {   // column i of cells: cell column i & 1 of quadrant column i >> 1
            const float x0 = (float)(i * 4 - QX * 4);
            if (lo > x0 + 3.f || hi < x0) continue;
            mask |= 1u << (4 * ((r >> 1) * QX + (i >> 1)) + 2 * (r & 1) + (i & 1));
        }
    }
    return mask;
}

}  // namespace sr
