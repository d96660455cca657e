// cell_cull_host.cpp -- host build of the staging lane's cell culling (streetunveiler_amd/csrc/footprint_cull.h), held to the blend
// kernels' own acceptance rule at every pixel centre of a 16x16 tile.  Built and run by tests/test_cell_cull_host.py:
//     c++ -O1 -std=c++17 -I <repo>/streetunveiler_amd/csrc tests/cell_cull_host.cpp -o cell_cull_host && ./cell_cull_host [seed]
// (also with -fsanitize=address,undefined: a stand-alone program).  For a few thousand seeded splats it restates stage_entry's
// A / B / C and intersect()'s float expressions (blend_common.h), marks the 4x4 cells that hold an accepted pixel -- alpha >= 1/255 with
// rho = min(rho3d, rho2d) -- and compares them with the cells the slab-extent test (cell_mask_rows) and the octagon test
// (cell_mask_octagon) keep, for the whole tile (<2, 2>) and for its two 16x8 bands (<2, 1> with the bands' yshift, what the row-mapped
// forward stages with).  Prints one JSON line; exit status 1 if the slab-extent test dropped a cell with an accepted pixel.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "footprint_cull.h"

namespace {

constexpr float kFilterInvSquare = 2.0f, kAlphaCap = 0.99f, kAlphaFloor = 1.0f / 255.0f, kLog2e = 1.4426950408889634f;   // common.h / blend_common.h

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uni() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }              // [0, 1)
    float range(float a, float b) { return a + (b - a) * uni(); }
    float logrange(float a, float b) { return a * powf(b / a, uni()); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Splat { float Tu[3], Tv[3], Tw[3], mx, my, opacity; };

// rows of the homography pixel ~ M (u, v, 1)^T in tile-local pixels: centre (px, py) at depth w, axes of s1 / s2 pixels (one sigma) at
// angle th, perspective terms g1 / g2 (the third row's share of u, v, per sigma)
Splat make(float px, float py, float w, float s1, float s2, float th, float g1, float g2, float opacity) {
    const float c = cosf(th), s = sinf(th);
    if (s1 == 0.f) g1 = 0.f;   // a zero scale zeroes its whole column of M, as in the pipeline (exact zeros: the p.z == 0 case of stage_entry)
    if (s2 == 0.f) g2 = 0.f;
    Splat sp;
    sp.Tw[0] = w * g1; sp.Tw[1] = w * g2; sp.Tw[2] = w;
    sp.Tu[0] = w * s1 * c + px * sp.Tw[0]; sp.Tu[1] = -w * s2 * s + px * sp.Tw[1]; sp.Tu[2] = px * w;
    sp.Tv[0] = w * s1 * s + py * sp.Tw[0]; sp.Tv[1] = w * s2 * c + py * sp.Tw[1]; sp.Tv[2] = py * w;
    sp.mx = px; sp.my = py; sp.opacity = opacity;
    return sp;
}

// the sixteen cells of the tile (bit 4 q + c, as cell_mask_rows<2, 2>) that hold a pixel the blend would accept
uint32_t accepted_cells(const Splat& sp, int* n_pixels) {
    const float *Tu = sp.Tu, *Tv = sp.Tv, *Tw = sp.Tw;
    const float A[3] = {Tv[1] * Tw[2] - Tv[2] * Tw[1], Tv[2] * Tw[0] - Tv[0] * Tw[2], Tv[0] * Tw[1] - Tv[1] * Tw[0]};
    const float B[3] = {Tw[1] * Tu[2] - Tw[2] * Tu[1], Tw[2] * Tu[0] - Tw[0] * Tu[2], Tw[0] * Tu[1] - Tw[1] * Tu[0]};
    const float C[3] = {Tu[1] * Tv[2] - Tu[2] * Tv[1], Tu[2] * Tv[0] - Tu[0] * Tv[2], Tu[0] * Tv[1] - Tu[1] * Tv[0]};
    const bool plane_degenerate = A[2] == 0.f && B[2] == 0.f && C[2] == 0.f;
    const float opacity = plane_degenerate ? 0.f : sp.opacity;
    uint32_t cells = 0;
    for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x) {
            const float xl = (float)(x - 8), yl = (float)(y - 8);
            const float ppx = fmaf(xl, A[0], fmaf(yl, B[0], C[0]));
            const float ppy = fmaf(xl, A[1], fmaf(yl, B[1], C[1]));
            const float ppz = fmaf(xl, A[2], fmaf(yl, B[2], C[2]));
            const float pz_inv = 1.f / ppz;
            const float sx = ppx * pz_inv, sy = ppy * pz_inv;
            const float rho3d = sx * sx + sy * sy;
            const float dx = sp.mx - xl, dy = sp.my - yl;
            const float rho2d = kFilterInvSquare * (dx * dx + dy * dy);
            const float rho = fminf(rho3d, rho2d);
            const float G = exp2f(rho * (-0.5f * kLog2e));
            const float alpha = fminf(kAlphaCap, opacity * G);
            if (alpha < kAlphaFloor) continue;   // (the depth and p.z tests of intersect() only drop more)
            ++*n_pixels;
            cells |= 1u << (4 * ((y >> 3) * 2 + (x >> 3)) + 2 * ((y >> 2) & 1) + ((x >> 2) & 1));
        }
    return cells;
}

struct Tally { long splats = 0, accepted = 0, kept_slab = 0, kept_oct = 0, false_slab = 0, false_oct = 0, missed_slab = 0, missed_oct = 0, missed_band = 0, band_differs = 0; };

int popc(uint32_t x) { return __builtin_popcount(x); }

void check(const Splat& sp, Tally& t, Tally& all) {
    int n_pixels = 0;
    const uint32_t hit = accepted_cells(sp, &n_pixels);
    const uint32_t slab = sr::cell_mask_rows<2, 2>(sp.Tu, sp.Tv, sp.Tw, sp.mx, sp.my, sp.opacity, 0.f);
    const uint32_t oct = sr::cell_mask_octagon<2, 2>(sp.Tu, sp.Tv, sp.Tw, sp.mx, sp.my, sp.opacity, 0.f);
    // the two band waves of the tile: quadrants 0, 1 at yshift -4 and quadrants 2, 3 at yshift +4
    const uint32_t band = sr::cell_mask_rows<2, 1>(sp.Tu, sp.Tv, sp.Tw, sp.mx, sp.my, sp.opacity, -4.f) |
                          (sr::cell_mask_rows<2, 1>(sp.Tu, sp.Tv, sp.Tw, sp.mx, sp.my, sp.opacity, 4.f) << 8);
    for (Tally* k : {&t, &all}) {
        k->splats += 1; k->accepted += popc(hit); k->kept_slab += popc(slab); k->kept_oct += popc(oct);
        k->false_slab += popc(slab & ~hit); k->false_oct += popc(oct & ~hit);
        k->missed_slab += popc(hit & ~slab); k->missed_oct += popc(hit & ~oct); k->missed_band += popc(hit & ~band);
        k->band_differs += popc(band ^ slab);
    }
    if ((hit & ~slab) | (hit & ~band))
        fprintf(stderr, "DROPPED: hit %04x slab %04x band %04x octagon %04x | Tu %g %g %g Tv %g %g %g Tw %g %g %g m %g %g opacity %g\n", hit, slab, band, oct,
                sp.Tu[0], sp.Tu[1], sp.Tu[2], sp.Tv[0], sp.Tv[1], sp.Tv[2], sp.Tw[0], sp.Tw[1], sp.Tw[2], sp.mx, sp.my, sp.opacity);
}

void print(const char* name, const Tally& t, bool last) {
    printf("\"%s\": {\"splats\": %ld, \"accepted_cells\": %ld, \"kept_slab\": %ld, \"kept_octagon\": %ld, \"false_slab\": %ld, \"false_octagon\": %ld, "
           "\"missed_slab\": %ld, \"missed_band\": %ld, \"missed_octagon\": %ld, \"band_differs\": %ld}%s",
           name, t.splats, t.accepted, t.kept_slab, t.kept_oct, t.false_slab, t.false_oct, t.missed_slab, t.missed_band, t.missed_oct, t.band_differs, last ? "" : ", ");
}

}  // namespace

int main(int argc, char** argv) {
    Rng r{argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull};
    const int N = argc > 2 ? atoi(argv[2]) : 600;   // splats per family
    const float kPi = 3.14159265f;
    Tally all;
    auto opacity = [&]() {   // 1/255 .. 1, the ends included; now and then just below the floor (an empty footprint)
        const int k = r.below(12);
        if (k == 0) return 1.f / 255.f;
        if (k == 1) return 1.f;
        if (k == 2) return 0.0039f;
        return r.logrange(1.f / 255.f, 1.f);
    };
    auto persp = [&]() { return r.below(3) == 0 ? 0.f : r.range(-0.03f, 0.03f); };
    auto depth = [&]() { return r.logrange(0.3f, 80.f); };
    printf("{");
    {   // isotropic
        Tally t;
        for (int i = 0; i < N; ++i) {
            const float s = r.logrange(0.05f, 15.f);
            check(make(r.range(-14.f, 14.f), r.range(-14.f, 14.f), depth(), s, s, r.range(0.f, kPi), persp(), persp(), opacity()), t, all);
        }
        print("isotropic", t, false);
    }
    {   // 20 : 1 at 0, 45, 90, 135 degrees and at arbitrary angles
        Tally t;
        for (int i = 0; i < 2 * N; ++i) {
            const float s = r.logrange(1.f, 60.f);
            const int k = r.below(8);
            const float th = k < 4 ? (float)k * (kPi / 4.f) : r.range(0.f, kPi);
            check(make(r.range(-20.f, 20.f), r.range(-20.f, 20.f), depth(), s, s / 20.f, th, persp(), persp(), opacity()), t, all);
        }
        print("elongated", t, false);
    }
    {   // centres far outside the tile, sized and turned so that many still reach it
        Tally t;
        for (int i = 0; i < N; ++i) {
            const float dist = r.logrange(30.f, 4000.f), dir = r.range(0.f, 2.f * kPi);
            const float s = dist * r.range(0.15f, 0.6f);
            const float th = r.below(2) ? dir + r.range(-0.05f, 0.05f) : r.range(0.f, kPi);
            check(make(dist * cosf(dir), dist * sinf(dir), depth(), s, s / r.logrange(1.f, 50.f), th, persp() * 0.02f, persp() * 0.02f, opacity()), t, all);
        }
        print("far_centres", t, false);
    }
    {   // c22 = w^2 (thr (g1^2 + g2^2) - 1) near zero from both sides: the cutoff disc almost reaches, or just crosses, the camera plane
        Tally t;
        for (int i = 0; i < N; ++i) {
            const float o = opacity();
            const float thr = fmaxf((2.f * logf(255.f * o)) * 1.01f + 0.01f, 0.01f);
            const float f = r.below(2) ? r.range(0.9f, 1.1f) : 1.f + r.range(-1e-3f, 1e-3f);
            const float a = r.range(0.f, 2.f * kPi), g = f / sqrtf(thr);
            const float s = r.logrange(0.5f, 20.f);
            check(make(r.range(-12.f, 12.f), r.range(-12.f, 12.f), depth(), s, s / r.logrange(1.f, 20.f), r.range(0.f, kPi), g * cosf(a), g * sinf(a), o), t, all);
        }
        print("c22_near_zero", t, false);
    }
    {   // zero scale: one axis, or both
        Tally t;
        for (int i = 0; i < N / 2; ++i) {
            const float s = r.logrange(0.5f, 20.f);
            const int k = r.below(3);
            check(make(r.range(-10.f, 10.f), r.range(-10.f, 10.f), depth(), k == 0 ? 0.f : s, k == 1 ? 0.f : (k == 2 ? s : 0.f), r.range(0.f, kPi), persp(), persp(), opacity()), t, all);
        }
        print("zero_scale", t, false);
    }
    {   // NaN and inf in the rows, the centre or the opacity: the blend's test lets a NaN alpha through at every pixel, so every cell must
        // be kept (opacity, where it is not the bad slot, from 1/255 up: below it the footprint is empty by definition, NaN rows or not)
        Tally t;
        for (int i = 0; i < N / 2; ++i) {
            const float s = r.logrange(0.5f, 20.f);
            Splat sp = make(r.range(-10.f, 10.f), r.range(-10.f, 10.f), depth(), s, s / r.logrange(1.f, 20.f), r.range(0.f, kPi), persp(), persp(), r.logrange(1.f / 255.f, 1.f));
            float* slots[12] = {&sp.Tu[0], &sp.Tu[1], &sp.Tu[2], &sp.Tv[0], &sp.Tv[1], &sp.Tv[2], &sp.Tw[0], &sp.Tw[1], &sp.Tw[2], &sp.mx, &sp.my, &sp.opacity};
            const float bad[3] = {NAN, INFINITY, -INFINITY};
            for (int n = 1 + r.below(3); n > 0; --n) *slots[r.below(12)] = bad[r.below(3)];
            check(sp, t, all);
        }
        print("nan_inf", t, false);
    }
    print("all", all, true);
    printf("}\n");
    return (all.missed_slab || all.missed_band) ? 1 : 0;   // (the octagon is the yardstick here: its counts are reported, the test reads them)
}
