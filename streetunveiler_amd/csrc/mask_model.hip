// mask_model.hip -- the getters of the reference's masked re-optimisation model (scene/mask_gaussian.py:139-176) and their adjoint:
//   masked_rows_kernel<false>   compose:   out = base + (mask[row] ? delta : 0.0f) for the six properties of every Gaussian, the two SH
//                               parts written into one [P,M,3] tensor; a fixed property (no delta) is its base
//   masked_rows_kernel<true>    backward:  d_delta = mask[row] ? upstream : 0.0f, the features' gradient split back into dc and rest
//
// Both are one statement: every OUTPUT tensor is walked as a flat stream of elements (stores are contiguous), element (row, col) of an
// output with row_len columns is read from source a for col < cut and from source b behind it, at row * pitch + off + (col [- cut]).
// A row with mask == 0 never has its delta (compose) or its upstream gradient (backward) read: what those rows hold -- NaN included --
// does not reach the output.  This file is built with -ffp-contract=off; the only arithmetic is one float32 add.
//
// A pure stream: no LDS, no atomics.  The outputs of a launch are cut into chunks of kMaskChunk elements; a workgroup walks chunks
// grid-stride and finds the output of a chunk as adam_step_kernel does, by selects over the (at most 6) first-chunk numbers of the table.
// An output whose pointer is 16-B aligned is written 16 B per lane (its n mod 4 tail as scalars); a source that is the same flat stream
// as its output (one source, pitch == row_len, 16-B aligned pointers) is read 16 B per lane too -- the delta only where all four rows
// of the group are selected.  Everything else (the SH halves, whose rows of 3, 27 or 45 floats end anywhere; a tensor that starts off a
// 16-B boundary) moves as scalars.
#include "abi.h"

namespace sr {

constexpr int kMaskThreads = 256;
constexpr int kMaskUnroll = 4;                                   // independent 16-B groups per thread
constexpr int kMaskChunk = kMaskThreads * 4 * kMaskUnroll;       // 4096 elements per workgroup iteration
constexpr int kMaskMaxBlocks = 2048;                             // 256 CUs x 8 workgroups; the rest is grid-strided
constexpr int kMaskSegments = 6;

struct MaskSrc {
    const float* p;          // compose: base;  backward: the upstream gradient
    const float* q;          // compose: delta, or nullptr for a fixed property;  backward: unused
    uint32_t pitch, off;     // element (row, c) of this source lies at row * pitch + off + c
};
struct MaskSeg {
    float* out;              // [rows, row_len], contiguous
    MaskSrc a, b;            // columns [0, cut) come from a, [cut, row_len) from b
    uint32_t row_len, cut;
    uint32_t n;              // rows * row_len
    uint32_t first_chunk;    // chunks of the launch in front of this output; 0xFFFFFFFF for an unused slot
    uint32_t out_vec;        // out is 16-B aligned
    uint32_t src_vec;        // one source that is the same flat stream as out, its pointers 16-B aligned
};
struct MaskTable {
    MaskSeg seg[kMaskSegments];
    const uint8_t* mask;     // [rows]
    uint32_t total_chunks;
};

template <bool BACKWARD>
__device__ __forceinline__ float masked_value(const float* p, const float* q, size_t at, bool selected) {
    if (BACKWARD) return selected ? p[at] : 0.0f;
    if (!q) return p[at];                                  // a fixed property is its base, bit for bit
    return p[at] + (selected ? q[at] : 0.0f);
}

// output element (row, col) from whichever source holds its column
template <bool BACKWARD>
__device__ __forceinline__ float masked_element(const MaskSeg& s, const uint8_t* mask, uint32_t row, uint32_t col) {
    const bool in_a = col < s.cut;
    const float* p = in_a ? s.a.p : s.b.p;
    const float* q = in_a ? s.a.q : s.b.q;
    const size_t at = (size_t)row * (in_a ? s.a.pitch : s.b.pitch) + (in_a ? s.a.off + col : s.b.off + (col - s.cut));
    return masked_value<BACKWARD>(p, q, at, (BACKWARD || q) && mask[row] != 0);
}

// one chunk of a 16-B aligned output: every lane owns groups of four consecutive elements
template <bool BACKWARD>
__device__ __forceinline__ void masked_chunk_vec(const MaskSeg& s, const uint8_t* mask, uint32_t base) {
#pragma unroll
    for (int u = 0; u < kMaskUnroll; ++u) {
        const uint32_t e = base + 4u * (u * kMaskThreads + threadIdx.x);
        if (e >= s.n) continue;
        uint32_t row = e / s.row_len, col = e - row * s.row_len;
        if (e + 4 > s.n) {                                  // the n mod 4 tail: one lane, at most three elements
            for (uint32_t i = e; i < s.n; ++i) {
                s.out[i] = masked_element<BACKWARD>(s, mask, row, col);
                if (++col == s.row_len) { col = 0; ++row; }
            }
            continue;
        }
        float v[4];
        if (s.src_vec) {                                    // source and output are the same flat stream
            bool sel[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sel[j] = (BACKWARD || s.a.q) && mask[row] != 0;
                if (++col == s.row_len) { col = 0; ++row; }
            }
            const bool all = sel[0] && sel[1] && sel[2] && sel[3], any = sel[0] || sel[1] || sel[2] || sel[3];
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BACKWARD) {
                float4 g = zero;
                if (all) g = *reinterpret_cast<const float4*>(s.a.p + e);
                else if (any) { if (sel[0]) g.x = s.a.p[e]; if (sel[1]) g.y = s.a.p[e + 1]; if (sel[2]) g.z = s.a.p[e + 2]; if (sel[3]) g.w = s.a.p[e + 3]; }
                v[0] = g.x; v[1] = g.y; v[2] = g.z; v[3] = g.w;
            } else {
                const float4 p = *reinterpret_cast<const float4*>(s.a.p + e);
                float4 d = zero;
                if (all) d = *reinterpret_cast<const float4*>(s.a.q + e);
                else if (any) { if (sel[0]) d.x = s.a.q[e]; if (sel[1]) d.y = s.a.q[e + 1]; if (sel[2]) d.z = s.a.q[e + 2]; if (sel[3]) d.w = s.a.q[e + 3]; }
                if (s.a.q) { v[0] = p.x + d.x; v[1] = p.y + d.y; v[2] = p.z + d.z; v[3] = p.w + d.w; }
                else { v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = masked_element<BACKWARD>(s, mask, row, col);
                if (++col == s.row_len) { col = 0; ++row; }
            }
        }
        *reinterpret_cast<float4*>(s.out + e) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// one chunk of an output that is only 4-B aligned: consecutive lanes, consecutive elements
template <bool BACKWARD>
__device__ __forceinline__ void masked_chunk_scalar(const MaskSeg& s, const uint8_t* mask, uint32_t base) {
#pragma unroll 4
    for (int k = 0; k < kMaskChunk / kMaskThreads; ++k) {
        const uint32_t e = base + k * kMaskThreads + threadIdx.x;
        if (e < s.n) {
            const uint32_t row = e / s.row_len;
            s.out[e] = masked_element<BACKWARD>(s, mask, row, e - row * s.row_len);
        }
    }
}

template <bool BACKWARD>
__global__ __launch_bounds__(kMaskThreads) void masked_rows_kernel(const MaskTable t) {
    for (uint32_t c = blockIdx.x; c < t.total_chunks; c += gridDim.x) {
        MaskSeg s = t.seg[0];
#pragma unroll
        for (int k = 1; k < kMaskSegments; ++k)
            if (c >= t.seg[k].first_chunk) s = t.seg[k];   // first_chunk ascends; unused slots hold 0xFFFFFFFF
        const uint32_t base = (c - s.first_chunk) * (uint32_t)kMaskChunk;
        if (s.out_vec) masked_chunk_vec<BACKWARD>(s, t.mask, base);
        else masked_chunk_scalar<BACKWARD>(s, t.mask, base);
    }
}

namespace {

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

struct TableBuilder {
    MaskTable t{};
    int used = 0;
    uint32_t chunks = 0;
    // an output of `rows` rows: columns [0, cut) from a, the rest from b; a zero-sized output is skipped
    void add(float* out, int rows, uint32_t row_len, uint32_t cut, MaskSrc a, MaskSrc b) {
        if (!out || rows == 0 || row_len == 0) return;
        MaskSeg& s = t.seg[used++];
        s.out = out; s.a = a; s.b = b; s.row_len = row_len; s.cut = cut;
        s.n = (uint32_t)rows * row_len;
        s.first_chunk = chunks;
        s.out_vec = aligned16(out);
        s.src_vec = cut == row_len && a.pitch == row_len && a.off == 0 && aligned16(a.p) && aligned16(a.q);
        chunks += (s.n + kMaskChunk - 1) / kMaskChunk;
    }
    template <bool BACKWARD>
    hipError_t launch(const uint8_t* mask, hipStream_t stream) {
        if (chunks == 0) return hipSuccess;
        for (int k = used; k < kMaskSegments; ++k) t.seg[k].first_chunk = 0xFFFFFFFFu;
        t.mask = mask;
        t.total_chunks = chunks;
        const uint32_t grid = chunks < (uint32_t)kMaskMaxBlocks ? chunks : (uint32_t)kMaskMaxBlocks;
        hipLaunchKernelGGL(masked_rows_kernel<BACKWARD>, dim3(grid), dim3(kMaskThreads), 0, stream, t);
        return hipGetLastError();
    }
};

bool mask_model_supported(int P, int M) { return (unsigned long long)P * 3ull * (unsigned long long)M < 0x7FFFFFFFull; }

// a NULL output / gradient pointer is skipped; a delta whose SR_MASK_FIXED_* bit is set is not read
hipError_t launch_mask_compose(int P, int M, const SrMaskTensors& base, const SrMaskTensors& delta, const uint8_t* mask, uint32_t fixed_bits,
                               const SrMaskEffective& out, hipStream_t stream) {
    const uint32_t rest = 3u * (uint32_t)(M - 1);
    auto src = [&](const float* p, const float* q, uint32_t bit, uint32_t pitch) { return MaskSrc{p, (fixed_bits & bit) ? nullptr : q, pitch, 0u}; };
    const MaskSrc none{nullptr, nullptr, 0u, 0u};
    TableBuilder b;
    b.add(out.xyz, P, 3, 3, src(base.xyz, delta.xyz, SR_MASK_FIXED_XYZ, 3), none);
    b.add(out.features, P, 3 + rest, 3, src(base.features_dc, delta.features_dc, SR_MASK_FIXED_FEATURES_DC, 3),
          src(base.features_rest, delta.features_rest, SR_MASK_FIXED_FEATURES_REST, rest));
    b.add(out.opacity, P, 1, 1, src(base.opacity, delta.opacity, SR_MASK_FIXED_OPACITY, 1), none);
    b.add(out.scaling, P, 2, 2, src(base.scaling, delta.scaling, SR_MASK_FIXED_SCALING, 2), none);
    b.add(out.rotation, P, 4, 4, src(base.rotation, delta.rotation, SR_MASK_FIXED_ROTATION, 4), none);
    return b.launch<false>(mask, stream);
}

hipError_t launch_mask_compose_backward(int P, int M, const SrMaskEffective& upstream, const uint8_t* mask, const SrMaskTensors& d,
                                        hipStream_t stream) {
    const uint32_t rest = 3u * (uint32_t)(M - 1), pitch = 3u * (uint32_t)M;
    const MaskSrc none{nullptr, nullptr, 0u, 0u};
    TableBuilder b;
    b.add(d.xyz, P, 3, 3, MaskSrc{upstream.xyz, nullptr, 3u, 0u}, none);
    b.add(d.features_dc, P, 3, 3, MaskSrc{upstream.features, nullptr, pitch, 0u}, none);
    b.add(d.features_rest, P, rest, rest, MaskSrc{upstream.features, nullptr, pitch, 3u}, none);
    b.add(d.opacity, P, 1, 1, MaskSrc{upstream.opacity, nullptr, 1u, 0u}, none);
    b.add(d.scaling, P, 2, 2, MaskSrc{upstream.scaling, nullptr, 2u, 0u}, none);
    b.add(d.rotation, P, 4, 4, MaskSrc{upstream.rotation, nullptr, 4u, 0u}, none);
    return b.launch<true>(mask, stream);
}

}  // namespace

}  // namespace sr

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
using namespace sr;

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

extern "C" {

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

}  // extern "C"
