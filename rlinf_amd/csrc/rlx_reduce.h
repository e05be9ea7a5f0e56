// rlx_reduce.h -- the two-stage streaming reduction every loss / statistics kernel is built on, in ONE place:
//   pass 1   a grid-stride loop accumulates K doubles per thread, store_partials<K> writes the block's row of `partials`
//   pass 2   one block: fold_partials<K> adds the rows, thread 0 finishes
// The summation order is part of the contract (the golden and float64 tests depend on it) and is defined here and nowhere else:
// lanes by xor butterfly (offsets 32 .. 1), waves in ascending order by thread 0, rows strided by the block's thread count.
// Included by rlx_common.h: no file includes it directly.
#pragma once

#include <algorithm>

#include "rlx_common.h"

namespace rlx {

// ---- host side ------------------------------------------------------------------------------------------------------------
constexpr int kPartialBlocks = 1024;  // rows of a partials workspace: the most blocks a first pass may have

// Blocks of a grid-stride pass over `work` items at `per_block` items per block and trip: enough to cover the work once,
// at most four per CU and at most `max_blocks` (the rows the partials workspace holds), at least one.
inline int stream_grid(long long work, int per_block = 256, int max_blocks = kPartialBlocks) {
    const long long want = (work + per_block - 1) / per_block;
    return (int)std::max<long long>(1, std::min<long long>(want, std::min<long long>(max_blocks, (long long)num_cu() * 4)));
}

#define RLX_REQUIRE_SPACE(have, need, who)                         \
    do {                                                           \
        if ((have) < (need)) {                                     \
            ::rlx::set_error("%s: workspace too small", (who));    \
            return RLX_ENOSPC;                                     \
        }                                                          \
    } while (0)

// ---- device side ----------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

template <typename T>  // double, float or long long
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, RLX_WAVE);
    return v;
}

// Block-wide sum of K doubles per thread.  `scratch` must hold K * (blockDim.x/64) doubles.
// Result valid in thread 0 only.  Deterministic (fixed tree).
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if (nw == 1) return;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) scratch[wid * K + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += scratch[w * K + k];
            v[k] = s;
        }
    }
}

// End of pass 1: block_sum, then thread 0 writes the block's row of partials[gridDim.x][K].
template <int K>
__device__ __forceinline__ void store_partials(double (&acc)[K], double* scratch, double* partials) {
    block_sum<K>(acc, scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partials[(size_t)blockIdx.x * K + k] = acc[k];
    }
}

// Pass 2: acc = the sum of the `nparts` rows of partials[nparts][K] -- thread t adds rows t, t + blockDim.x, ... in ascending
// order, slots in ascending k, then block_sum.  Result valid in thread 0 only.
template <int K>
__device__ __forceinline__ void fold_partials(const double* partials, int nparts, double (&acc)[K], double* scratch) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partials[(size_t)i * K + k];
    }
    block_sum<K>(acc, scratch);
}

__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }

// Block-wide maximum of K values per thread, float or double: wave butterfly, one value per wave through LDS, thread 0 folds
// the waves in ascending order.  `scratch` must hold K * (blockDim.x/64) values and be free (the caller synchronises before it
// is written again).  Result valid in thread 0 only.  A minimum goes in negated: min(a, b) == -max(-a, -b) bit for bit, signed
// zeros and NaNs included.
template <typename T, int K>
__device__ __forceinline__ void block_max(T (&v)[K], T* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = max_of(v[k], __shfl_xor(v[k], off, RLX_WAVE));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) scratch[wid * K + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = max_of(v[k], scratch[w * K + k]);
        }
    }
}

#endif  // __HIPCC__

}  // namespace rlx
