// rollout_store.hip -- the two device passes of the async-PPO rollout store (rlinf/workers/actor/async_ppo_fsdp_worker.py:112-182,
// rlinf/data/storage/replay/buffer.py:1129-1199, rlinf/data/schema/embodied_types.py:500-559).
//
//   rlx_version_stats          one pass over a trajectory's `versions`: min, exact integer sum of the rounded versions, and the
//                              histogram of round_half_even(v) -- what the store's priority (min, mean) and get_metric need, in one
//                              small struct the host reads back once per added trajectory (the reference does .min().item(),
//                              .mean().item() per add and torch.unique per stored trajectory per get_metric call).
//   rlx_gather_rows_segmented  torch.cat(dim=1) over S stored trajectories + flatten + row gather as ONE pass: the concatenated
//                              copy of the large fields is never written or re-read.
//
// Both are HBM-bound streaming kernels.  Integer arithmetic only in the reductions (two-stage, fixed tree): deterministic.

#include <algorithm>

#include "rlx_common.h"

namespace rlx {
namespace {

// ---- version statistics ------------------------------------------------------------------------------------------------------
// A partial (one per block of stage 1) is a row of int64: [min bits, sum, below, above, count[0 .. n_bins)].
constexpr int VS_HEAD = 4;
constexpr int VS_THREADS = 256;
constexpr int VS_MAX_BLOCKS = 1024;

struct VsRun {  // the run of equal bins a thread is in: a trajectory is sampled with one or two versions, so a thread's elements
    int bin;    // almost always fall into one bin and the LDS histogram sees one atomic per thread instead of one per element
    unsigned long long cnt;
};

__device__ __forceinline__ void vs_flush(const VsRun& r, unsigned long long* hist, int n_bins) {
    if (r.cnt == 0) return;
    const int slot = r.bin < 0 ? n_bins : (r.bin >= n_bins ? n_bins + 1 : r.bin);  // [n_bins] = below, [n_bins + 1] = above
    atomicAdd(&hist[slot], r.cnt);
}

__device__ __forceinline__ void vs_take(float v, long long base, int n_bins, float& vmin, long long& sum, VsRun& run,
                                        unsigned long long* hist) {
    vmin = fminf(vmin, v);
    const long long r = (long long)rintf(v);  // round half to even: torch.round (buffer.py:1185)
    sum += r;
    const long long d = r - base;
    const int bin = d < 0 ? -1 : (d >= n_bins ? n_bins : (int)d);
    if (bin != run.bin) {
        vs_flush(run, hist, n_bins);
        run.bin = bin;
        run.cnt = 0;
    }
    ++run.cnt;
}

__global__ __launch_bounds__(VS_THREADS) void version_stats_partial_kernel(const float* __restrict__ v, long long n, long long base,
                                                                           int n_bins, long long* __restrict__ partials) {
    __shared__ unsigned long long hist[RLX_VERSION_STATS_MAX_BINS + 2];
    __shared__ float s_min[VS_THREADS / RLX_WAVE];
    __shared__ long long s_sum[VS_THREADS / RLX_WAVE];
    for (int k = threadIdx.x; k < n_bins + 2; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    float vmin = __int_as_float(0x7f800000);  // +inf
    long long sum = 0;
    VsRun run{-2, 0};
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    // 16-byte loads over the aligned body, scalar head and tail
    const uintptr_t addr = reinterpret_cast<uintptr_t>(v);
    long long head = (long long)(((16 - (addr & 15)) & 15) / 4);
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v + head);
    for (long long i = tid; i < n4; i += stride) {
        const float4 q = v4[i];
        vs_take(q.x, base, n_bins, vmin, sum, run, hist);
        vs_take(q.y, base, n_bins, vmin, sum, run, hist);
        vs_take(q.z, base, n_bins, vmin, sum, run, hist);
        vs_take(q.w, base, n_bins, vmin, sum, run, hist);
    }
    const long long tail0 = head + n4 * 4;
    for (long long i = tid; i < head + (n - tail0); i += stride)
        vs_take(i < head ? v[i] : v[tail0 + (i - head)], base, n_bins, vmin, sum, run, hist);
    vs_flush(run, hist, n_bins);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmin = fminf(vmin, __shfl_xor(vmin, off, RLX_WAVE));
    sum = wave_sum(sum);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        s_min[wid] = vmin;
        s_sum[wid] = sum;
    }
    __syncthreads();
    long long* row = partials + (long long)blockIdx.x * (VS_HEAD + n_bins);
    if (threadIdx.x == 0) {
        float m = s_min[0];
        long long s = s_sum[0];
        for (int w = 1; w < VS_THREADS / RLX_WAVE; ++w) {
            m = fminf(m, s_min[w]);
            s += s_sum[w];
        }
        row[0] = (long long)__float_as_int(m);
        row[1] = s;
        row[2] = (long long)hist[n_bins];
        row[3] = (long long)hist[n_bins + 1];
    }
    for (int k = threadIdx.x; k < n_bins; k += blockDim.x) row[VS_HEAD + k] = (long long)hist[k];
}

// one block: column k of the partial matrix is summed (min for column 0) by thread k, in block order
__global__ __launch_bounds__(128) void version_stats_final_kernel(const long long* __restrict__ partials, int n_partials, long long n,
                                                                  long long base, int n_bins, rlx_version_stats_out* __restrict__ out) {
    const int k = threadIdx.x, width = VS_HEAD + n_bins;
    if (k >= width) return;
    if (k == 0) {
        float m = __int_as_float(0x7f800000);
        for (int p = 0; p < n_partials; ++p) m = fminf(m, __int_as_float((int)partials[(long long)p * width]));
        out->min = m;
        out->n_bins = n_bins;
        out->n = n;
        out->base = base;
        return;
    }
    long long s = 0;
    for (int p = 0; p < n_partials; ++p) s += partials[(long long)p * width + k];
    if (k == 1) out->sum = s;
    else if (k == 2) out->below = s;
    else if (k == 3) out->above = s;
    else out->count[k - VS_HEAD] = s;
}

int vs_blocks(long long n) {
    // >= 16 elements (four 16-byte loads) per thread before a second block pays
    return stream_grid(n, VS_THREADS * 16, VS_MAX_BLOCKS);
}

// ---- segmented gather --------------------------------------------------------------------------------------------------------
struct SegField {
    const char* src[RLX_STORE_MAX_SLOTS];
    char* dst;
    long long row_bytes;
    long long t_rows;
    int word_bytes;  // 16 / 8 / 4 / 1: the widest word every slot pointer, the destination and the row size are aligned to
};

struct SegArgs {
    SegField f[RLX_GATHER_MAX_FIELDS];
    long long off[RLX_STORE_MAX_SLOTS + 1];  // prefix sums of the per-slot env counts; off[n_slots] = sum B
    const int64_t* index;                    // nullptr: the plain concatenation, every field over its own t_rows * sum B rows
    long long n_rows;                        // rows per field with an index
    int n_slots;
};

// grid.y = field; each thread moves one word of one destination row.  idx_t = uint32_t when every product fits (the usual case:
// 64-bit divisions cost an order of magnitude more ALU than the 16 bytes they place).
template <typename word_t, typename idx_t>
__device__ __forceinline__ void seg_field(const SegArgs& a, const SegField& fd) {
    const idx_t wpr = (idx_t)(fd.row_bytes / (long long)sizeof(word_t));
    const idx_t sum_b = (idx_t)a.off[a.n_slots];
    const idx_t rows = a.index ? (idx_t)a.n_rows : (idx_t)fd.t_rows * sum_b;
    const idx_t total = rows * wpr;
    const idx_t stride = (idx_t)gridDim.x * blockDim.x;
    const idx_t t_rows = (idx_t)fd.t_rows;
    word_t* __restrict__ dst = reinterpret_cast<word_t*>(fd.dst);
    for (idx_t i = (idx_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const idx_t row = i / wpr, w = i - row * wpr;
        idx_t t, b;
        if (a.index) {
            const unsigned long long j = (unsigned long long)a.index[row];
            if (j >= (unsigned long long)t_rows * sum_b) continue;  // an index outside the field (negative ones included): nothing is read
            const idx_t jj = (idx_t)j;
            t = jj / sum_b;
            b = jj - t * sum_b;
        } else {
            t = row / sum_b;
            b = row - t * sum_b;
        }
        // the slot that holds env b: a uniform walk over the (scalar) table, selected per lane -- no divergent table index
        const char* base = fd.src[0];
        idx_t lo = 0, width = (idx_t)a.off[1];
        for (int s = 1; s < a.n_slots; ++s) {
            const idx_t o = (idx_t)a.off[s];
            if (b >= o) {
                base = fd.src[s];
                lo = o;
                width = (idx_t)a.off[s + 1] - o;
            }
        }
        const unsigned long long src_row = (unsigned long long)t * width + (b - lo);
        dst[i] = reinterpret_cast<const word_t*>(base + src_row * (unsigned long long)fd.row_bytes)[w];
    }
}

template <typename idx_t>
__global__ __launch_bounds__(256) void gather_rows_segmented_kernel(SegArgs a) {
    const SegField& fd = a.f[blockIdx.y];
    if (fd.word_bytes == 16) seg_field<uint4, idx_t>(a, fd);
    else if (fd.word_bytes == 8) seg_field<uint2, idx_t>(a, fd);
    else if (fd.word_bytes == 4) seg_field<uint32_t, idx_t>(a, fd);
    else seg_field<uint8_t, idx_t>(a, fd);
}

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" size_t rlx_version_stats_workspace_bytes(int64_t n) {
    (void)n;
    return (size_t)VS_MAX_BLOCKS * (VS_HEAD + RLX_VERSION_STATS_MAX_BINS) * sizeof(long long);
}

extern "C" int rlx_version_stats(const float* versions, int64_t n, int64_t base, int n_bins, rlx_version_stats_out* out, void* workspace,
                                 size_t workspace_bytes, rlx_stream_t stream) {
    RLX_REQUIRE(n >= 1, "rlx_version_stats: n=%lld (a trajectory has at least one version)", (long long)n);
    RLX_REQUIRE(n_bins >= 1 && n_bins <= RLX_VERSION_STATS_MAX_BINS, "rlx_version_stats: n_bins=%d (1..%d)", n_bins,
                RLX_VERSION_STATS_MAX_BINS);
    RLX_REQUIRE(versions && out && workspace, "rlx_version_stats: NULL argument");
    RLX_REQUIRE(reinterpret_cast<uintptr_t>(versions) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                "rlx_version_stats: misaligned pointer");
    if (workspace_bytes < rlx_version_stats_workspace_bytes(n)) {
        set_error("rlx_version_stats: workspace of %zu bytes, needs %zu", workspace_bytes, rlx_version_stats_workspace_bytes(n));
        return RLX_ENOSPC;
    }
    const int blocks = vs_blocks(n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(version_stats_partial_kernel, dim3(blocks), dim3(VS_THREADS), 0, st, versions, (long long)n, (long long)base,
                       n_bins, static_cast<long long*>(workspace));
    RLX_LAUNCH_CHECK();
    hipLaunchKernelGGL(version_stats_final_kernel, dim3(1), dim3(128), 0, st, static_cast<const long long*>(workspace), blocks,
                       (long long)n, (long long)base, n_bins, out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_gather_rows_segmented(const rlx_seg_field* fields, int n_fields, int n_slots, const int64_t* slot_envs,
                                         const int64_t* index, int64_t n_rows, rlx_stream_t stream) {
    RLX_REQUIRE(n_fields >= 0 && n_fields <= RLX_GATHER_MAX_FIELDS, "rlx_gather_rows_segmented: n_fields=%d (max %d)", n_fields,
                RLX_GATHER_MAX_FIELDS);
    RLX_REQUIRE(n_slots >= 1 && n_slots <= RLX_STORE_MAX_SLOTS, "rlx_gather_rows_segmented: n_slots=%d (1..%d)", n_slots,
                RLX_STORE_MAX_SLOTS);
    RLX_REQUIRE(n_rows >= 0, "rlx_gather_rows_segmented: negative n_rows");
    RLX_REQUIRE(slot_envs != nullptr, "rlx_gather_rows_segmented: NULL slot_envs table");
    SegArgs a;
    a.off[0] = 0;
    for (int s = 0; s < n_slots; ++s) {
        RLX_REQUIRE(slot_envs[s] > 0, "rlx_gather_rows_segmented: slot %d holds B_s=%lld envs", s, (long long)slot_envs[s]);
        a.off[s + 1] = a.off[s] + slot_envs[s];
    }
    for (int s = n_slots; s < RLX_STORE_MAX_SLOTS; ++s) a.off[s + 1] = a.off[n_slots];
    if (n_fields == 0 || (index != nullptr && n_rows == 0)) return RLX_OK;
    RLX_REQUIRE(fields != nullptr, "rlx_gather_rows_segmented: NULL field table");
    const long long sum_b = a.off[n_slots];
    long long max_threads = 0, max_total = 0;
    for (int i = 0; i < n_fields; ++i) {
        const rlx_seg_field& f = fields[i];
        RLX_REQUIRE(f.srcs != nullptr && f.dst != nullptr, "rlx_gather_rows_segmented: field %d has a NULL table or destination", i);
        RLX_REQUIRE(f.row_bytes > 0, "rlx_gather_rows_segmented: field %d has row_bytes=%lld", i, (long long)f.row_bytes);
        RLX_REQUIRE(f.t_rows > 0, "rlx_gather_rows_segmented: field %d has t_rows=%lld", i, (long long)f.t_rows);
        SegField& d = a.f[i];
        uintptr_t align = reinterpret_cast<uintptr_t>(f.dst) | (uintptr_t)f.row_bytes;
        for (int s = 0; s < n_slots; ++s) {
            RLX_REQUIRE(f.srcs[s] != nullptr, "rlx_gather_rows_segmented: field %d, slot %d is NULL", i, s);
            d.src[s] = static_cast<const char*>(f.srcs[s]);
            align |= reinterpret_cast<uintptr_t>(f.srcs[s]);
        }
        for (int s = n_slots; s < RLX_STORE_MAX_SLOTS; ++s) d.src[s] = nullptr;
        d.dst = static_cast<char*>(f.dst);
        d.row_bytes = f.row_bytes;
        d.t_rows = f.t_rows;
        d.word_bytes = align % 16 == 0 ? 16 : (align % 8 == 0 ? 8 : (align % 4 == 0 ? 4 : 1));
        const long long rows = index ? (long long)n_rows : (long long)f.t_rows * sum_b;
        max_threads = std::max(max_threads, rows * ((f.row_bytes + 3) / 4));
        // the 32-bit form: word counts (at the narrowest word the field could take) and flat row numbers below 2^31
        max_total = std::max({max_total, rows * f.row_bytes, (long long)f.t_rows * sum_b});
    }
    a.index = index;
    a.n_rows = n_rows;
    a.n_slots = n_slots;
    const int gx = (int)std::max<long long>(1, std::min<long long>((max_threads + 255) / 256, (long long)num_cu() * 8));
    // grid-stride loop counters stay below 2^32 in the 32-bit form: i + stride <= total + gx * 256
    if (max_total + (long long)gx * 256 < (1ll << 31))
        hipLaunchKernelGGL(gather_rows_segmented_kernel<uint32_t>, dim3(gx, n_fields), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(gather_rows_segmented_kernel<unsigned long long>, dim3(gx, n_fields), dim3(256), 0,
                           static_cast<hipStream_t>(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
