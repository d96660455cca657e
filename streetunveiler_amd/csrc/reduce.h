// reduce.h -- the fixed-order sum of the auxiliary losses (aux_loss.hip), written once for its three ops:
//   block_sum          every workgroup folds its threads' terms in the LDS, always pairing the same slots, and thread 0 gets the sum;
//   finalize_sums<K>   ONE workgroup adds the K interleaved columns of per-block partials, thread t taking blocks t, t + T, t + 2T, ...,
//                      then the same fold.
// Everything is a double: a term is the float64 expression of its float32 inputs, so the one rounding of a loss is the last store.
// No atomics: the order of every addition is a function of the element count alone, two calls on equal inputs give equal bits.
#pragma once
#include "common.h"

namespace sr {

constexpr int kReduceThreads = 256;   // workgroup size of the term kernels AND of the finalize workgroup

// sum of v over the kReduceThreads threads of the workgroup; valid in thread 0.  `red` is kReduceThreads doubles of LDS; the leading
// barrier lets a caller use it twice in a row.
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// sums[k] = the sum over i < n_blocks of partials[K * i + k]; valid in thread 0 of the one workgroup that calls it
template <int K>
__device__ __forceinline__ void finalize_sums(const double* __restrict__ partials, int n_blocks, double* red, double (&sums)[K]) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (size_t i = threadIdx.x; i < (size_t)n_blocks; i += kReduceThreads) {   // (size_t: n_blocks may be within a stride of INT_MAX)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partials[K * i + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sums[k] = block_sum(acc[k], red);
}

}  // namespace sr
