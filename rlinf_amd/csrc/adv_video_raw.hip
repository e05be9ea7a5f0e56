// adv_video_raw.hip -- the last two names of the advantage registry, "grpo_video" and "raw", gfx950.
//
// Replaces:
//   compute_grpo_video_advantages  rlinf/algorithms/advantages.py:124-164  (embodied only; the dispatcher skips the score scan)
//   compute_raw_advantages         rlinf/algorithms/advantages.py:410-438  (embodied after calculate_scores, and reasoning)
// on the layouts the callers hold: embodied [n_chunk, B, C] with element (n, b, c) = step n * C + c of env b, reasoning
// [bsz, seq].  Nothing is transposed or copied.
//
//   * video_frame_kernel: advantage_mode "frame".  One thread owns one group -- the G rewards of (step, prompt), G floats at
//     stride C -- and makes one pass: mean and unbiased variance in f64 (two passes over the thread's own values), then
//     (r - mean) / (std + eps) rounded to f32 once and multiplied by the mask.  C == 1 with G in {4, 8, 16} (16-byte aligned
//     buffers) keeps the group in registers: G / 4 float4 loads, G mask bytes in one load, G / 4 float4 stores.  Every other
//     (G, C) re-reads its group from the cache (the lines are shared with the neighbouring lanes), so HBM traffic stays
//     4 + 1 B read and 4 B written per element.
//   * video_video_kernel: advantage_mode "video".  ONE launch, one workgroup per prompt.  The prompt's N = T * G rewards
//     (n_chunk blocks of G * C contiguous floats, B * C apart) are visited in the order k = t * G + g, t = n * C + c -- the
//     order of the reference's [T, B] view -- so a [n_chunk, B, C] buffer and its flattened [T, B, 1] view sum in the same
//     order and give the same bits.  N <= kVideoLdsFloats (8192 floats = 32 KB of the CU's 160 KB, so several prompts share a
//     CU; the contract shape needs 128 x 8 = 1024) keeps the rewards in LDS between the moment phases and the write; a larger
//     prompt reads its rewards again for each phase (from L2 where they fit).
//   * raw_counts_kernel + raw_write_kernel: adv = score[b] * mask over (outer, batch, inner) = (n_chunk, B, C) or
//     (1, bsz, seq).  Un-normalised: raw_write_kernel alone, 1 B read and 4 B written per element.  Normalised: every value
//     is score[b] * mask, so the masked moments need the mask only.  raw_counts_kernel gives every workgroup a fixed tile of
//     envs, counts their mask bytes as integers (LDS), and writes (count, sum, sum of squares) of the tile as three doubles:
//     sum_b cnt[b] * d[b], sum_b cnt[b] * d[b]^2 with d = score[b] - pivot (pivot = score[0]: shifted data, so identical scores
//     give a variance of exactly 0, as torch's two-pass std does).  Integer counts do not depend on the layout and the tiles
//     depend on `batch` only, so (n_chunk, B, C) and its [T, B, 1] view give the same bits.  raw_write_kernel: every
//     workgroup folds the (at most a few hundred) tile records in index order, forms mean and 1 / (std + eps) in f64, and
//     streams 16 mask bytes in, 4 float4 out per lane (flat over the buffer; with fewer than 16 steps per env and row --
//     embodied -- a lane owns 16 columns, forms their values once and walks its rows: raw_write_cols_kernel).  TWO launches rather than
//     gae_scan.hip's "block 0 finishes the moments once and publishes them" form: there the waiting workgroups wait for
//     partials the SAME launch order has already produced; here the records come from a different decomposition (env tiles
//     over all rows) than the write (a flat stream), so one launch would need a grid-wide phase change, i.e. workgroups
//     spinning on others that may not be resident.  The second launch costs a few microseconds at a latency-bound shape and
//     nothing measurable at a bandwidth-bound one, and every workgroup folding a few hundred records is 12 KB of L2 reads.
// Moments are f64 sums in a fixed order (lane-strided partial sums, a fixed butterfly, waves in index order): no float
// atomics, no dependence on which workgroup arrives first; two runs give the same bits.
// Masked positions are value * 0 in the reference's sense (+0.0 / -0.0 by the sign of the value, NaN where it is NaN).

#include "rlx_common.h"

namespace rlx {
namespace {

constexpr int kThreads = 256;
constexpr int kVideoLdsFloats = 8192;
constexpr int kRawTileTarget = 512;   // raw_counts: about this many env tiles (= moment records)
constexpr int kRawTileMinEnvs = 16;
constexpr int kRawTileMaxEnvs = 4096;  // ints of LDS per tile

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned_dev(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// (v - mean) * inv in f64, rounded to f32 once, times the mask
__device__ __forceinline__ float norm_mul(float v, double mean, double inv, bool keep) {
    return fmul((float)(((double)v - mean) * inv), keep ? 1.f : 0.f);
}

// ---- grpo_video, frame ------------------------------------------------------------------------------------------------------
// GV > 0: C == 1 and G == GV, registers.  GV == 0: any G, C.
template <int GV>
__global__ __launch_bounds__(kThreads) void video_frame_kernel(const float* __restrict__ r, const uint8_t* __restrict__ m,
                                                               float* __restrict__ adv, long long n_groups, int B, int C, int G,
                                                               float eps) {
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n_groups) return;
    if constexpr (GV > 0) {
        const size_t base = (size_t)gid * GV;
        float v[GV];
        uint8_t mk[GV];
#pragma unroll
        for (int q = 0; q < GV / 4; ++q) {
            const v4f x = *reinterpret_cast<const v4f*>(r + base + 4 * q);
            const unsigned w = *reinterpret_cast<const unsigned*>(m + base + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = x[j], mk[4 * q + j] = (uint8_t)((w >> (8 * j)) & 0xffu);
        }
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < GV; ++j) sum += (double)v[j];
        const double mean = sum / (double)GV;
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            const double d = (double)v[j] - mean;
            ss += d * d;
        }
        const double inv = 1.0 / (sqrt(ss / (double)(GV - 1)) + (double)eps);
#pragma unroll
        for (int q = 0; q < GV / 4; ++q) {
            v4f y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = norm_mul(v[4 * q + j], mean, inv, mk[4 * q + j] != 0);
            *reinterpret_cast<v4f*>(adv + base + 4 * q) = y;
        }
    } else {
        const long long P = B / G;
        const int c = (int)(gid % C);
        const long long pn = gid / C;
        const long long p = pn % P, nn = pn / P;
        const size_t base = ((size_t)nn * B + (size_t)p * G) * C + c;
        double sum = 0.0;
        for (int j = 0; j < G; ++j) sum += (double)r[base + (size_t)j * C];
        const double mean = sum / (double)G;
        double ss = 0.0;
        for (int j = 0; j < G; ++j) {
            const double d = (double)r[base + (size_t)j * C] - mean;
            ss += d * d;
        }
        const double inv = 1.0 / (sqrt(ss / (double)(G - 1)) + (double)eps);  // G == 1: 0 / 0 -> NaN everywhere, as torch.std
        for (int j = 0; j < G; ++j) {
            const size_t i = base + (size_t)j * C;
            adv[i] = norm_mul(r[i], mean, inv, m[i] != 0);
        }
    }
}

// ---- grpo_video, video ------------------------------------------------------------------------------------------------------
// block-wide f64 sum, the result in every thread (fixed tree)
__device__ __forceinline__ double block_sum_all(double v, double* scratch) {
    double a[1] = {v};
    block_sum<1>(a, scratch);
    __syncthreads();
    if (threadIdx.x == 0) scratch[kThreads / 64] = a[0];
    __syncthreads();
    return scratch[kThreads / 64];
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void video_video_kernel(const float* __restrict__ r, const uint8_t* __restrict__ m,
                                                               float* __restrict__ adv, int n_chunk, int B, int C, int G,
                                                               float eps) {
    extern __shared__ float s_r[];
    __shared__ double s_red[kThreads / 64 + 1];
    const int N = n_chunk * C * G;  // (the host checks that this fits an int)
    const size_t p0 = (size_t)blockIdx.x * G;
    auto index_of = [&](int k) -> size_t {  // k = t * G + g, t = n * C + c
        const int t = k / G, g = k - t * G;
        if (C == 1) return ((size_t)t * B + p0 + g);
        const int nn = t / C, c = t - nn * C;
        return ((size_t)nn * B + p0 + g) * C + c;
    };
    double acc = 0.0;
    for (int k = threadIdx.x; k < N; k += kThreads) {
        const float v = r[index_of(k)];
        if constexpr (LDS) s_r[k] = v;
        acc += (double)v;
    }
    const double mean = block_sum_all(acc, s_red) / (double)N;
    acc = 0.0;
    for (int k = threadIdx.x; k < N; k += kThreads) {
        float v;
        if constexpr (LDS) v = s_r[k];  // (each thread reads back what it wrote itself)
        else v = r[index_of(k)];
        const double d = (double)v - mean;
        acc += d * d;
    }
    const double ss = block_sum_all(acc, s_red);
    const double inv = 1.0 / (sqrt(ss / (double)(N - 1)) + (double)eps);  // N == 1 -> NaN
    for (int k = threadIdx.x; k < N; k += kThreads) {
        const size_t i = index_of(k);
        float v;
        if constexpr (LDS) v = s_r[k];
        else v = r[i];
        adv[i] = norm_mul(v, mean, inv, m[i] != 0);
    }
}

// ---- raw --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float raw_pivot(const float* scores) {
    const float s0 = scores[0];
    return (s0 - s0 == 0.f) ? s0 : 0.f;  // a non-finite first score cannot serve as the shift
}

// Workgroup `tile` owns envs [tile * tile_envs, ...): integer mask counts per env in LDS, then one moment record.
__global__ __launch_bounds__(kThreads) void raw_counts_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ m,
                                                              double* __restrict__ records, long long outer, long long batch,
                                                              long long inner, int tile_envs) {
    extern __shared__ int s_cnt[];
    __shared__ double s_red[3 * (kThreads / 64)];
    const long long b_lo = (long long)blockIdx.x * tile_envs;
    const int nb = (int)min((long long)tile_envs, batch - b_lo);
    for (int i = threadIdx.x; i < nb; i += kThreads) s_cnt[i] = 0;
    __syncthreads();
    const long long L = (long long)nb * inner;          // contiguous mask bytes of this tile in one outer row
    const long long row_stride = batch * inner;
    const uint8_t* base = m + b_lo * inner;
    const bool vec = L % 16 == 0 && row_stride % 16 == 0 && aligned_dev(base, 16);
    if (vec) {
        const long long L16 = L / 16, units = outer * L16;
        for (long long u = threadIdx.x; u < units; u += kThreads) {
            const long long o = u / L16, q = (u - o * L16) * 16;
            const v4u w = *reinterpret_cast<const v4u*>(base + o * row_stride + q);
            long long e = q / inner;
            long long left = inner - (q - e * inner);  // bytes of env e from q on
            int run = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                run += ((w[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0u;
                if (--left == 0 || j == 15) {
                    if (run) atomicAdd(&s_cnt[e], run);  // (an integer LDS add: exact, order-free)
                    run = 0, ++e, left = inner;
                }
            }
        }
    } else {
        const long long total = outer * L;
        for (long long u = threadIdx.x; u < total; u += kThreads) {
            const long long o = u / L, q = u - o * L;
            if (base[o * row_stride + q]) atomicAdd(&s_cnt[q / inner], 1);
        }
    }
    __syncthreads();
    const double pivot = (double)raw_pivot(scores);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += kThreads) {
        const int c = s_cnt[i];
        if (c) {  // (an env without a valid element does not enter the moments, whatever its score)
            const double d = (double)scores[b_lo + i] - pivot, cd = (double)c;
            acc[0] += cd, acc[1] += cd * d, acc[2] += cd * d * d;
        }
    }
    block_sum<3>(acc, s_red);
    if (threadIdx.x == 0) {
        records[3 * (size_t)blockIdx.x + 0] = acc[0];
        records[3 * (size_t)blockIdx.x + 1] = acc[1];
        records[3 * (size_t)blockIdx.x + 2] = acc[2];
    }
}

// V == 16: 16-byte aligned buffers, units of 16 consecutive elements (+ a scalar tail); V == 1: any alignment.
template <bool NORM, int V>
__global__ __launch_bounds__(kThreads) void raw_write_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ m,
                                                             float* __restrict__ adv, const double* __restrict__ records,
                                                             int n_records, long long total, long long batch, long long inner,
                                                             float eps) {
    __shared__ double s_red[3 * (kThreads / 64)];
    __shared__ double s_mom[3];
    double mean = 0.0, inv = 0.0;
    bool norm = false;
    if constexpr (NORM) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n_records; i += kThreads) {
            acc[0] += records[3 * (size_t)i], acc[1] += records[3 * (size_t)i + 1], acc[2] += records[3 * (size_t)i + 2];
        }
        block_sum<3>(acc, s_red);
        if (threadIdx.x == 0) s_mom[0] = acc[0], s_mom[1] = acc[1], s_mom[2] = acc[2];
        __syncthreads();
        const double cnt = s_mom[0], sd1 = s_mom[1], sd2 = s_mom[2];
        norm = cnt > 0.0;  // "if valid.numel() > 0" (advantages.py:434)
        mean = (double)raw_pivot(scores) + sd1 / cnt;
        const double var = (sd2 - sd1 * sd1 / cnt) / (cnt - 1.0);  // unbiased; one valid element: 0 / 0 -> NaN, as torch.std
        inv = 1.0 / (sqrt(var > 0.0 || var != var ? var : 0.0) + (double)eps);
    }
    auto value = [&](float s, bool keep) -> float {
        const float a = fmul(s, keep ? 1.f : 0.f);
        if (!NORM || !norm) return a;
        return (float)(((double)a - mean) * inv);  // every element, masked ones included (advantages.py:435)
    };
    const long long stride = (long long)gridDim.x * kThreads;
    if constexpr (V == 16) {
        const long long units = total / 16;
        for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
            const long long i0 = u * 16;
            const v4u w = *reinterpret_cast<const v4u*>(m + i0);
            const long long row = i0 / inner;  // (outer, batch) row of the first element
            long long left = inner - (i0 - row * inner);
            long long b = row % batch;
            float s = scores[b];
            float v1 = value(s, true), v0 = value(s, false);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v4f y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = ((w[q] >> (8 * j)) & 0xffu) != 0u ? v1 : v0;
                    if (--left == 0 && (4 * q + j) < 15) {
                        left = inner;
                        if (++b == batch) b = 0;
                        s = scores[b];
                        v1 = value(s, true), v0 = value(s, false);
                    }
                }
                *reinterpret_cast<v4f*>(adv + i0 + 4 * q) = y;
            }
        }
        for (long long i = units * 16 + (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride)
            adv[i] = value(scores[(i / inner) % batch], m[i] != 0);
    } else {
        for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride)
            adv[i] = value(scores[(i / inner) % batch], m[i] != 0);
    }
}

// Few steps per env and row (embodied, inner < 16): the flat stream above would look a score up for almost every element.
// Here a thread owns 16 consecutive columns of the [outer][batch * inner] matrix, forms their two possible values once
// (scores are read as neighbours, coalesced) and then streams its rows: 16 mask bytes in, 4 float4 out per row.
// grid.x = column tiles, grid.y = row slabs.  Needs (batch * inner) % 16 == 0 and 16-byte aligned buffers.
template <bool NORM>
__global__ __launch_bounds__(kThreads) void raw_write_cols_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ m,
                                                                  float* __restrict__ adv, const double* __restrict__ records,
                                                                  int n_records, long long outer, long long ncol, int inner,
                                                                  int rows_per_block, float eps) {
    __shared__ double s_red[3 * (kThreads / 64)];
    __shared__ double s_mom[3];
    double mean = 0.0, inv = 0.0;
    bool norm = false;
    if constexpr (NORM) {  // (the same fold as raw_write_kernel: the same bits)
        double acc[3] = {0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < n_records; i += kThreads) {
            acc[0] += records[3 * (size_t)i], acc[1] += records[3 * (size_t)i + 1], acc[2] += records[3 * (size_t)i + 2];
        }
        block_sum<3>(acc, s_red);
        if (threadIdx.x == 0) s_mom[0] = acc[0], s_mom[1] = acc[1], s_mom[2] = acc[2];
        __syncthreads();
        const double cnt = s_mom[0], sd1 = s_mom[1], sd2 = s_mom[2];
        norm = cnt > 0.0;
        mean = (double)raw_pivot(scores) + sd1 / cnt;
        const double var = (sd2 - sd1 * sd1 / cnt) / (cnt - 1.0);
        inv = 1.0 / (sqrt(var > 0.0 || var != var ? var : 0.0) + (double)eps);
    }
    const long long col0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (col0 >= ncol) return;
    float v1[16], v0[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float s = scores[(col0 + j) / inner];
        const float a0 = fmul(s, 0.f);
        v1[j] = (NORM && norm) ? (float)(((double)s - mean) * inv) : s;
        v0[j] = (NORM && norm) ? (float)(((double)a0 - mean) * inv) : a0;
    }
    const long long k_lo = (long long)blockIdx.y * rows_per_block, k_hi = min(outer, k_lo + rows_per_block);
    for (long long k = k_lo; k < k_hi; ++k) {
        const size_t i0 = (size_t)k * ncol + col0;
        const v4u w = *reinterpret_cast<const v4u*>(m + i0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v4f y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = ((w[q] >> (8 * j)) & 0xffu) != 0u ? v1[4 * q + j] : v0[4 * q + j];
            *reinterpret_cast<v4f*>(adv + i0 + 4 * q) = y;
        }
    }
}

int raw_tile_envs(long long batch) {
    long long t = (batch + kRawTileTarget - 1) / kRawTileTarget;
    if (t < kRawTileMinEnvs) t = kRawTileMinEnvs;
    if (t > kRawTileMaxEnvs) t = kRawTileMaxEnvs;
    return (int)t;
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_grpo_video_adv(const float* rewards, const uint8_t* loss_mask, float* advantages, int n_chunk, int batch,
                                  int chunk, int group_size, int mode, float eps, rlx_stream_t stream) {
    RLX_REQUIRE(n_chunk >= 0 && batch >= 0 && chunk >= 1, "rlx_grpo_video_adv: bad sizes");
    RLX_REQUIRE(group_size >= 1 && batch % group_size == 0, "rlx_grpo_video_adv: batch %d %% group_size %d != 0", batch,
                group_size);
    RLX_REQUIRE(mode == RLX_GRPO_VIDEO_FRAME || mode == RLX_GRPO_VIDEO_VIDEO, "rlx_grpo_video_adv: mode %d", mode);
    if (batch == 0 || n_chunk == 0) return RLX_OK;
    RLX_REQUIRE(rewards && loss_mask && advantages, "rlx_grpo_video_adv: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == RLX_GRPO_VIDEO_FRAME) {
        const long long n_groups = (long long)n_chunk * (batch / group_size) * chunk;
        const long long blocks = (n_groups + kThreads - 1) / kThreads;
        RLX_REQUIRE(blocks < 0x7fffffffLL, "rlx_grpo_video_adv: %lld groups exceed the grid", n_groups);
        const bool regs = chunk == 1 && aligned(rewards, 16) && aligned(advantages, 16) && aligned(loss_mask, 4);
        const dim3 grid((unsigned)blocks), block(kThreads);
        if (regs && group_size == 4)
            hipLaunchKernelGGL(video_frame_kernel<4>, grid, block, 0, s, rewards, loss_mask, advantages, n_groups, batch, chunk,
                               group_size, eps);
        else if (regs && group_size == 8)
            hipLaunchKernelGGL(video_frame_kernel<8>, grid, block, 0, s, rewards, loss_mask, advantages, n_groups, batch, chunk,
                               group_size, eps);
        else if (regs && group_size == 16)
            hipLaunchKernelGGL(video_frame_kernel<16>, grid, block, 0, s, rewards, loss_mask, advantages, n_groups, batch, chunk,
                               group_size, eps);
        else
            hipLaunchKernelGGL(video_frame_kernel<0>, grid, block, 0, s, rewards, loss_mask, advantages, n_groups, batch, chunk,
                               group_size, eps);
    } else {
        const long long N = (long long)n_chunk * chunk * group_size;
        RLX_REQUIRE(N < 0x7fffffffLL, "rlx_grpo_video_adv: %lld rewards per prompt must be < 2^31", N);
        const dim3 grid((unsigned)(batch / group_size)), block(kThreads);
        if (N <= kVideoLdsFloats)
            hipLaunchKernelGGL(video_video_kernel<true>, grid, block, (size_t)N * sizeof(float), s, rewards, loss_mask, advantages,
                               n_chunk, batch, chunk, group_size, eps);
        else
            hipLaunchKernelGGL(video_video_kernel<false>, grid, block, 0, s, rewards, loss_mask, advantages, n_chunk, batch,
                               chunk, group_size, eps);
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" size_t rlx_raw_adv_workspace_bytes(int64_t outer, int64_t batch, int64_t inner) {
    (void)outer, (void)inner;
    if (batch <= 0) return 8;
    const long long tiles = (batch + raw_tile_envs(batch) - 1) / raw_tile_envs(batch);
    return (size_t)tiles * 3 * sizeof(double);
}

extern "C" int rlx_raw_adv(const float* scores, const uint8_t* loss_mask, float* advantages, int64_t outer, int64_t batch,
                           int64_t inner, int normalize, float eps, void* workspace, size_t workspace_bytes,
                           rlx_stream_t stream) {
    RLX_REQUIRE(outer >= 0 && batch >= 0 && inner >= 0, "rlx_raw_adv: negative size");
    RLX_REQUIRE(outer < 0x7fffffffLL && batch < 0x7fffffffLL && inner < 0x7fffffffLL &&
                    (batch == 0 || outer * inner <= 0x7fffffffffffffffLL / batch),
                "rlx_raw_adv: sizes too large");
    const long long total = outer * batch * inner;
    if (total == 0) return RLX_OK;
    RLX_REQUIRE(scores && loss_mask && advantages, "rlx_raw_adv: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double* records = nullptr;
    int n_records = 0;
    if (normalize) {
        const int tile_envs = raw_tile_envs(batch);
        n_records = (int)((batch + tile_envs - 1) / tile_envs);
        RLX_REQUIRE(workspace != nullptr && aligned(workspace, 8), "rlx_raw_adv: normalize needs an 8-byte aligned workspace");
        if (workspace_bytes < rlx_raw_adv_workspace_bytes(outer, batch, inner)) {
            set_error("rlx_raw_adv: workspace of %zu bytes, %zu needed", workspace_bytes,
                      rlx_raw_adv_workspace_bytes(outer, batch, inner));
            return RLX_ENOSPC;
        }
        hipLaunchKernelGGL(raw_counts_kernel, dim3((unsigned)n_records), dim3(kThreads), (size_t)tile_envs * sizeof(int), s, scores,
                           loss_mask, static_cast<double*>(workspace), (long long)outer, (long long)batch, (long long)inner,
                           tile_envs);
        RLX_LAUNCH_CHECK();
        records = static_cast<const double*>(workspace);
    }
    const long long ncol = batch * inner;
    if (inner < 16 && ncol % 16 == 0 && aligned(loss_mask, 16) && aligned(advantages, 16)) {
        const int gx = ceil_div(ncol / 16, kThreads);
        int gy = 1;
        while ((long long)gx * gy < 4LL * num_cu() && outer / (gy * 2) >= 2) gy *= 2;
        const int rows = ceil_div(outer, gy);
        const dim3 grid((unsigned)gx, (unsigned)ceil_div(outer, rows)), block(kThreads);
        RLX_REQUIRE(grid.y <= 65535u, "rlx_raw_adv: too many row slabs");
        if (normalize)
            hipLaunchKernelGGL(raw_write_cols_kernel<true>, grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               (long long)outer, ncol, (int)inner, rows, eps);
        else
            hipLaunchKernelGGL(raw_write_cols_kernel<false>, grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               (long long)outer, ncol, (int)inner, rows, eps);
        RLX_LAUNCH_CHECK();
        return RLX_OK;
    }
    const bool vec = aligned(loss_mask, 16) && aligned(advantages, 16) && total >= 16;
    const long long work = vec ? (total + 15) / 16 : total;
    long long blocks = (work + kThreads - 1) / kThreads;
    const long long cap = (long long)num_cu() * 16;
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (normalize) {
        if (vec)
            hipLaunchKernelGGL((raw_write_kernel<true, 16>), grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               total, (long long)batch, (long long)inner, eps);
        else
            hipLaunchKernelGGL((raw_write_kernel<true, 1>), grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               total, (long long)batch, (long long)inner, eps);
    } else {
        if (vec)
            hipLaunchKernelGGL((raw_write_kernel<false, 16>), grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               total, (long long)batch, (long long)inner, eps);
        else
            hipLaunchKernelGGL((raw_write_kernel<false, 1>), grid, block, 0, s, scores, loss_mask, advantages, records, n_records,
                               total, (long long)batch, (long long)inner, eps);
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
