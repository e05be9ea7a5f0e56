// grpo_dynamic.hip -- multi-turn GRPO advantages and the dynamic-batch loss scales, gfx950.
//
// Replaces:
//   compute_grpo_dynamic_advantages  rlinf/algorithms/advantages.py:167-299  (registry name "grpo_dynamic"), in the reasoning
//                                    dispatcher's [num_seq, seq] layout (utils.py:207-215,265-277)
//   group_scale / agent_scale / turn_scale  rlinf/algorithms/loss_scales.py  (registry names "group_level", "agent_level",
//                                    "turn_level", registry.py:128-147)
// The reference loops over turns in Python: one indexed-tensor op per turn for the advantages, one .item() per turn for the
// turn-level scale.  Here the host turns idx_to_traj into a CSR once (turn rows sorted stably by trajectory, trajectory
// offsets), and:
//   * grpo_dyn_adv_kernel: ONE launch.  Every workgroup covers a tile of one row; its wave 0 re-derives that row's advantage
//     from the CSR in a fixed order (the question's rewards, f64 sums folded by a fixed butterfly), so every workgroup of a row
//     gets the same bits without a workspace, atomics or a second launch.  The other waves have their mask loads in flight
//     meanwhile; then the tile is streamed: 4 mask bytes in, 4 values out per lane and vector.
//   * row_scale_kernel: x[row, :] *= f[row] (agent_level, per-row factors formed in f64 on the host and rounded to f32 once)
//     or x *= f (group_level) -- one f32 multiply per element, exactly torch's `t *= python_float`.
//   * turn_scale_kernel: one workgroup per (trajectory, sub-trajectory) group counts its rows' mask bytes, forms
//     T * |o_t| / sum |o_t| in f64 (the reference's Python int arithmetic, correctly rounded), rounds to f32 and scales the rows.
//     A group whose total is 0 scales nothing and raises a flag (the reference raises ZeroDivisionError there).
// Rows start wherever row * seq puts them: each row is split into a scalar head up to the first 4-aligned flat index, 4-wide
// vectors and a scalar tail, so any seq (1, odd, 7097) takes the vector path for its body.

#include <algorithm>

#include "rlx_common.h"
#include "rlx_convert.h"

namespace rlx {
namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;   // elements per lane and vector: 4 mask bytes, 16 B of f32 (8 B of bf16)
constexpr int kVpt = 8;   // vectors per lane per tile
constexpr int kTileVecs = kThreads * kVpt;
constexpr int kCntCap = 1024;  // turn_scale: row counts of a group kept in LDS (larger groups recount)

struct RowSplit {
    long long head, nv, tail0, tail;
    __device__ __forceinline__ RowSplit(long long rb, long long seq) {
        head = (kVec - rb % kVec) % kVec;
        if (head > seq) head = seq;
        nv = (seq - head) / kVec;
        tail0 = head + nv * kVec;
        tail = seq - tail0;
    }
};

// the value the reference holds after an op in the rewards' dtype
template <typename R>
__device__ __forceinline__ float rnd(float v) {
    return (float)Conv<float, R>::cvt(v);
}
template <>
__device__ __forceinline__ float rnd<float>(float v) {
    return v;
}

template <typename T>
struct Io4;
template <>
struct Io4<float> {
    static __device__ __forceinline__ void load(const float* p, float (&x)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&x)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    }
};
template <>
struct Io4<__bf16> {
    static __device__ __forceinline__ void load(const __bf16* p, float (&x)[4]) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        x[0] = __uint_as_float(q.x << 16), x[1] = __uint_as_float(q.x & 0xffff0000u);
        x[2] = __uint_as_float(q.y << 16), x[3] = __uint_as_float(q.y & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(__bf16* p, const float (&x)[4]) {
        uint16_t h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const __bf16 b = Conv<float, __bf16>::cvt(x[i]);
            h[i] = *reinterpret_cast<const uint16_t*>(&b);
        }
        *reinterpret_cast<uint2*>(p) = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
    }
};

__device__ __forceinline__ double wave_bcast_sum(double v) { return __shfl(wave_sum(v), 0, RLX_WAVE); }

// Trajectory tr's reward: its turns' rewards summed in turn order in the rewards' dtype (trajectory_rewards[traj] += r), then
// divided in f32 by max(count, 1) (advantages.py:239-246).
template <typename R>
__device__ __forceinline__ float traj_reward(const R* rewards, const int* order, const int* off, int tr) {
    const int lo = off[tr], hi = off[tr + 1];
    float acc = 0.f;
    for (int i = lo; i < hi; ++i) acc = rnd<R>(acc + (float)rewards[order[i]]);
    return acc / (float)max(hi - lo, 1);
}

// The advantage of `row`, in the value the reference stores into turn_advantages (the rewards' dtype).  Called by all 64 lanes
// of one wave; the result is valid in every lane.
template <typename R>
__device__ float dyn_adv(const R* rewards, const int* traj_of_row, const int* order, const int* off, long long row, int G,
                         int mode, float eps) {
    const int lane = threadIdx.x & 63;
    const int q0 = (traj_of_row[row] / G) * G;
    double s = 0.0, ss = 0.0, n;
    float self;
    if (mode == RLX_GRPO_DYN_TURN) {  // mean / unbiased std over every turn of the question (advantages.py:268-287)
        const int lo = off[q0], hi = off[q0 + G];
        n = (double)(hi - lo);
        for (int i = lo + lane; i < hi; i += RLX_WAVE) s += (double)(float)rewards[order[i]];
        const double mean = wave_bcast_sum(s) / n;
        for (int i = lo + lane; i < hi; i += RLX_WAVE) {
            const double d = (double)(float)rewards[order[i]] - mean;
            ss += d * d;
        }
        ss = wave_bcast_sum(ss);
        const float mean_f = rnd<R>((float)mean);
        const float std_f = rnd<R>((float)sqrt(ss / (n - 1.0)));  // a single turn: 0 / 0 = NaN, as torch.std
        self = (float)rewards[row];
        const float d = rnd<R>(fsub(self, mean_f));
        return rnd<R>(d / rnd<R>(fadd(std_f, eps)));
    }
    // trajectory mode: mean / unbiased std over the question's group_size trajectory rewards (advantages.py:248-263)
    n = (double)G;
    for (int k = lane; k < G; k += RLX_WAVE) s += (double)traj_reward(rewards, order, off, q0 + k);
    const double mean = wave_bcast_sum(s) / n;
    for (int k = lane; k < G; k += RLX_WAVE) {
        const double d = (double)traj_reward(rewards, order, off, q0 + k) - mean;
        ss += d * d;
    }
    ss = wave_bcast_sum(ss);
    const float mean_f = (float)mean, std_f = (float)sqrt(ss / (n - 1.0));
    self = traj_reward(rewards, order, off, traj_of_row[row]);
    return rnd<R>(fsub(self, mean_f) / fadd(std_f, eps));  // f32 from the division on; stored in the rewards' dtype
}

// grid: num_seq * tiles workgroups; workgroup (row, tile) writes the tile's vectors, tile 0 the head, the last tile the tail.
template <typename R>
__global__ __launch_bounds__(kThreads) void grpo_dyn_adv_kernel(const R* __restrict__ rewards, const int* __restrict__ plan,
                                                                const uint8_t* __restrict__ m, R* __restrict__ out,
                                                                long long num_seq, long long num_traj, long long seq,
                                                                int tiles, int G, int mode, float eps) {
    __shared__ float s_adv;
    const long long row = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(row * tiles);
    const int* traj_of_row = plan;
    const int* order = plan + num_seq;
    const int* off = plan + 2 * num_seq;
    const long long rb = row * seq;
    const RowSplit sp(rb, seq);
    const uint8_t* mrow = m + rb;
    const long long v0 = (long long)tile * kTileVecs + threadIdx.x;
    uint32_t mw[kVpt];
#pragma unroll
    for (int k = 0; k < kVpt; ++k) {
        const long long v = v0 + (long long)k * kThreads;
        mw[k] = v < sp.nv ? *reinterpret_cast<const uint32_t*>(mrow + sp.head + v * kVec) : 0u;
    }
    if (threadIdx.x < RLX_WAVE) {
        const float a = dyn_adv<R>(rewards, traj_of_row, order, off, row, G, mode, eps);
        if (threadIdx.x == 0) s_adv = a;
    }
    __syncthreads();
    const float a = s_adv;
    R* orow = out + rb;
#pragma unroll
    for (int k = 0; k < kVpt; ++k) {
        const long long v = v0 + (long long)k * kThreads;
        if (v < sp.nv) {
            float x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = fmul(a, ((mw[k] >> (8 * i)) & 0xffu) ? 1.f : 0.f);  // multiply: NaN stays, -0.0
            Io4<R>::store(orow + sp.head + v * kVec, x);
        }
    }
    if (tile == 0 && threadIdx.x < sp.head) orow[threadIdx.x] = Conv<float, R>::cvt(fmul(a, mrow[threadIdx.x] ? 1.f : 0.f));
    if (tile == tiles - 1 && threadIdx.x < sp.tail) {
        const long long j = sp.tail0 + threadIdx.x;
        orow[j] = Conv<float, R>::cvt(fmul(a, mrow[j] ? 1.f : 0.f));
    }
}

template <typename T>
__device__ __forceinline__ T scale1(T x, float f) {
    return Conv<float, T>::cvt(fmul((float)x, f));
}

// x[row, :] *= (row_factor ? row_factor[row] : factor);  grid: rows * tiles
template <typename T>
__global__ __launch_bounds__(kThreads) void row_scale_kernel(T* __restrict__ x, const float* __restrict__ row_factor, float factor,
                                                             long long seq, int tiles) {
    const long long row = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(row * tiles);
    const float f = row_factor ? row_factor[row] : factor;
    const long long rb = row * seq;
    const RowSplit sp(rb, seq);
    T* xr = x + rb;
    const long long v0 = (long long)tile * kTileVecs + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < kVpt; ++k) {
        const long long v = v0 + (long long)k * kThreads;
        if (v < sp.nv) {
            float e[4];
            Io4<T>::load(xr + sp.head + v * kVec, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = fmul(e[i], f);
            Io4<T>::store(xr + sp.head + v * kVec, e);
        }
    }
    if (tile == 0 && threadIdx.x < sp.head) xr[threadIdx.x] = scale1(xr[threadIdx.x], f);
    if (tile == tiles - 1 && threadIdx.x < sp.tail) xr[sp.tail0 + threadIdx.x] = scale1(xr[sp.tail0 + threadIdx.x], f);
}

__device__ __forceinline__ int nonzero_bytes(uint32_t w) {
    return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u);
}

// number of nonzero mask bytes of row `row` (response_mask[row].sum()); every thread of the block gets it
__device__ long long count_row(const uint8_t* m, long long row, long long seq, long long* s_part) {
    const long long rb = row * seq;
    const RowSplit sp(rb, seq);
    const uint8_t* mr = m + rb;
    long long c = 0;
    for (long long v = threadIdx.x; v < sp.nv; v += kThreads) c += nonzero_bytes(*reinterpret_cast<const uint32_t*>(mr + sp.head + v * kVec));
    if (threadIdx.x < sp.head) c += mr[threadIdx.x] != 0;
    if (threadIdx.x < sp.tail) c += mr[sp.tail0 + threadIdx.x] != 0;
    c = wave_sum(c);
    __syncthreads();  // the previous row's partials have been read
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    long long t = 0;
#pragma unroll
    for (int w = 0; w < kThreads / RLX_WAVE; ++w) t += s_part[w];
    return t;
}

// grid: one workgroup per (trajectory, sub-trajectory) group; plan = order[num_seq] | group offsets[num_groups + 1]
template <typename T>
__global__ __launch_bounds__(kThreads) void turn_scale_kernel(T* __restrict__ x, const uint8_t* __restrict__ m,
                                                              const int* __restrict__ plan, long long num_seq, long long seq,
                                                              int* __restrict__ zero_flag) {
    __shared__ long long s_part[kThreads / RLX_WAVE];
    __shared__ long long s_cnt[kCntCap];
    const int* order = plan;
    const int* off = plan + num_seq;
    const int lo = off[blockIdx.x], n_turns = off[blockIdx.x + 1] - lo;
    long long total = 0;
    for (int k = 0; k < n_turns; ++k) {
        const long long c = count_row(m, order[lo + k], seq, s_part);
        if (k < kCntCap && threadIdx.x == 0) s_cnt[k] = c;
        total += c;
    }
    if (total == 0) {  // masked_count_all == 0: the reference's division raises; leave the rows as they are
        if (threadIdx.x == 0) *zero_flag = 1;
        return;
    }
    __syncthreads();  // s_cnt
    for (int k = 0; k < n_turns; ++k) {
        const long long c = k < kCntCap ? s_cnt[k] : count_row(m, order[lo + k], seq, s_part);
        // 1 * len(sub_traj_idxes) * masked_counts[i] / masked_count_all: exact integers, one correctly rounded division
        const float f = (float)((double)((long long)n_turns * c) / (double)total);
        const long long rb = (long long)order[lo + k] * seq;
        const RowSplit sp(rb, seq);
        T* xr = x + rb;
        for (long long v = threadIdx.x; v < sp.nv; v += kThreads) {
            float e[4];
            Io4<T>::load(xr + sp.head + v * kVec, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = fmul(e[i], f);
            Io4<T>::store(xr + sp.head + v * kVec, e);
        }
        if (threadIdx.x < sp.head) xr[threadIdx.x] = scale1(xr[threadIdx.x], f);
        if (threadIdx.x < sp.tail) xr[sp.tail0 + threadIdx.x] = scale1(xr[sp.tail0 + threadIdx.x], f);
    }
}

int tiles_of(long long seq) {
    const long long nv_max = seq / kVec;
    return (int)std::max<long long>(1, (nv_max + kTileVecs - 1) / kTileVecs);
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_grpo_dynamic_adv(const void* rewards, int rewards_dtype, const int32_t* plan, const uint8_t* loss_mask,
                                    void* advantages, int64_t num_seq, int64_t num_traj, int64_t seq, int group_size, int mode,
                                    float eps, rlx_stream_t stream) {
    RLX_REQUIRE(num_seq >= 0 && num_traj >= 0 && seq >= 0, "rlx_grpo_dynamic_adv: negative size");
    RLX_REQUIRE(num_seq < 0x7fffffffLL && num_traj < 0x7fffffffLL, "rlx_grpo_dynamic_adv: num_seq / num_traj must be < 2^31");
    RLX_REQUIRE(group_size >= 1 && num_traj % group_size == 0, "rlx_grpo_dynamic_adv: num_traj %lld not divisible by group_size %d",
                (long long)num_traj, group_size);
    RLX_REQUIRE(mode == RLX_GRPO_DYN_TRAJECTORY || mode == RLX_GRPO_DYN_TURN, "rlx_grpo_dynamic_adv: mode %d", mode);
    if (num_seq == 0 || seq == 0) return RLX_OK;
    RLX_REQUIRE(rewards && plan && loss_mask && advantages, "rlx_grpo_dynamic_adv: NULL argument");
    RLX_REQUIRE(num_traj >= 1, "rlx_grpo_dynamic_adv: num_seq > 0 needs num_traj >= 1");
    const int tiles = tiles_of(seq);
    RLX_REQUIRE(num_seq * tiles < 0x7fffffffLL, "rlx_grpo_dynamic_adv: %lld rows x %d tiles exceed the grid", (long long)num_seq, tiles);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(num_seq * tiles));
    const int* p = reinterpret_cast<const int*>(plan);
    switch (rewards_dtype) {
        case RLX_DTYPE_F32:
            RLX_REQUIRE(aligned(loss_mask, 4) && aligned(advantages, 16), "rlx_grpo_dynamic_adv: loss_mask / advantages misaligned");
            hipLaunchKernelGGL(grpo_dyn_adv_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<const float*>(rewards), p,
                               loss_mask, static_cast<float*>(advantages), (long long)num_seq, (long long)num_traj,
                               (long long)seq, tiles, group_size, mode, eps);
            break;
        case RLX_DTYPE_BF16:
            RLX_REQUIRE(aligned(loss_mask, 4) && aligned(advantages, 8), "rlx_grpo_dynamic_adv: loss_mask / advantages misaligned");
            hipLaunchKernelGGL(grpo_dyn_adv_kernel<__bf16>, grid, dim3(kThreads), 0, s, static_cast<const __bf16*>(rewards), p,
                               loss_mask, static_cast<__bf16*>(advantages), (long long)num_seq, (long long)num_traj,
                               (long long)seq, tiles, group_size, mode, eps);
            break;
        default: set_error("rlx_grpo_dynamic_adv: rewards_dtype %d is not f32 / bf16", rewards_dtype); return RLX_EINVAL;
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_loss_scale_rows(void* x, int dtype, const float* row_factor, float factor, int64_t rows, int64_t cols,
                                   rlx_stream_t stream) {
    RLX_REQUIRE(rows >= 0 && cols >= 0, "rlx_loss_scale_rows: negative size");
    if (rows == 0 || cols == 0) return RLX_OK;
    RLX_REQUIRE(x != nullptr, "rlx_loss_scale_rows: NULL x");
    const int tiles = tiles_of(cols);
    RLX_REQUIRE(rows * tiles < 0x7fffffffLL, "rlx_loss_scale_rows: %lld rows x %d tiles exceed the grid", (long long)rows, tiles);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(rows * tiles));
    switch (dtype) {
        case RLX_DTYPE_F32:
            RLX_REQUIRE(aligned(x, 16), "rlx_loss_scale_rows: x must be 16-byte aligned");
            hipLaunchKernelGGL(row_scale_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<float*>(x), row_factor, factor,
                               (long long)cols, tiles);
            break;
        case RLX_DTYPE_BF16:
            RLX_REQUIRE(aligned(x, 8), "rlx_loss_scale_rows: x must be 8-byte aligned");
            hipLaunchKernelGGL(row_scale_kernel<__bf16>, grid, dim3(kThreads), 0, s, static_cast<__bf16*>(x), row_factor, factor,
                               (long long)cols, tiles);
            break;
        default: set_error("rlx_loss_scale_rows: dtype %d is not f32 / bf16", dtype); return RLX_EINVAL;
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_loss_scale_turn(void* loss_scales, int dtype, const uint8_t* response_mask, const int32_t* plan,
                                   int64_t num_seq, int64_t num_groups, int64_t seq, int32_t* zero_flag, rlx_stream_t stream) {
    RLX_REQUIRE(num_seq >= 0 && num_groups >= 0 && seq >= 0, "rlx_loss_scale_turn: negative size");
    RLX_REQUIRE(num_seq < 0x7fffffffLL && num_groups <= num_seq, "rlx_loss_scale_turn: num_seq >= 2^31 or more groups than rows");
    if (num_groups == 0) return RLX_OK;
    RLX_REQUIRE(loss_scales && response_mask && plan && zero_flag, "rlx_loss_scale_turn: NULL argument");
    RLX_REQUIRE(aligned(response_mask, 4), "rlx_loss_scale_turn: response_mask must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int* p = reinterpret_cast<const int*>(plan);
    switch (dtype) {
        case RLX_DTYPE_F32:
            RLX_REQUIRE(aligned(loss_scales, 16), "rlx_loss_scale_turn: loss_scales must be 16-byte aligned");
            hipLaunchKernelGGL(turn_scale_kernel<float>, dim3((unsigned)num_groups), dim3(kThreads), 0, s,
                               static_cast<float*>(loss_scales), response_mask, p, (long long)num_seq, (long long)seq, zero_flag);
            break;
        case RLX_DTYPE_BF16:
            RLX_REQUIRE(aligned(loss_scales, 8), "rlx_loss_scale_turn: loss_scales must be 8-byte aligned");
            hipLaunchKernelGGL(turn_scale_kernel<__bf16>, dim3((unsigned)num_groups), dim3(kThreads), 0, s,
                               static_cast<__bf16*>(loss_scales), response_mask, p, (long long)num_seq, (long long)seq, zero_flag);
            break;
        default: set_error("rlx_loss_scale_turn: dtype %d is not f32 / bf16", dtype); return RLX_EINVAL;
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
