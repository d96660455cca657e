// scan.h -- the prefix sums every kernel file shares (device code): over a wave, over a block, and over an array one block walks in
// chunks with a carry.  T is uint32_t or uint4 (four independent sums, component-wise: HIP's vector operators).
#pragma once
#include "common.h"

namespace sr {

// Inclusive prefix sum over the 64 lanes of a wave: DPP row shifts inside the rows of 16 lanes, then the two row broadcasts
// (six VALU instructions; __shfl_up goes through the LDS crossbar six times).  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);   // row_bcast:31 -> rows 2, 3
    return (uint32_t)v;
}
__device__ __forceinline__ uint4 wave_inclusive_scan(uint4 x) {
    return make_uint4(wave_inclusive_scan(x.x), wave_inclusive_scan(x.y), wave_inclusive_scan(x.z), wave_inclusive_scan(x.w));
}

// The cross-wave step of a block scan: `incl` = the inclusive scan of x inside the caller's wave; returns the exclusive prefix of x over
// the block's kWaves * 64 threads and, in `total`, the block's sum (to every thread).  s_w: kWaves words of LDS.  Two barriers, the
// first because s_w may still be in use by the scan before this one.  All threads of the block must call it.
template <int kWaves, class T>
__device__ inline T block_exclusive_from_waves(T incl, T x, T* s_w, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();   // s_w may still be in use
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    T off{}, tot{};
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { const T c = s_w[k]; if (k < w) off += c; tot += c; }
    total = tot;
    return off + incl - x;
}
// exclusive prefix of x over the block's threads (+ the block total)
template <int kWaves, class T>
__device__ inline T block_exclusive_scan(T x, T* s_w, T& total) {
    return block_exclusive_from_waves<kWaves>(wave_inclusive_scan(x), x, s_w, total);
}

// One block of kWaves * 64 threads scans row[0 .. n) in place (exclusive), a chunk of one item per thread at a time, the sum of the
// chunks so far carried in a register; returns the total to every thread.  Two barriers per chunk.
template <int kWaves, class T>
__device__ inline T carried_exclusive_scan(T* row, int n, T* s_w) {
    T carry{};
    for (int c = 0; c < n; c += kWaves * 64) {
        const int i = c + (int)threadIdx.x;
        const T x = i < n ? row[i] : T{};
        T total;
        const T excl = block_exclusive_scan<kWaves>(x, s_w, total);
        if (i < n) row[i] = carry + excl;
        carry += total;
    }
    return carry;
}

}  // namespace sr
