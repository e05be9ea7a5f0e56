// rlx_mlp_tile.h -- the 32-row tile GEMMs, head helpers and the split-K weight-gradient kernel that the 256-wide MLP model calls
// share (sac_mlp.hip, iql_mlp.hip).  Everything is in an unnamed namespace: each file that includes it gets its own kernels.
//   forward / backward-data: one workgroup (4 waves) owns a 32-row tile of the batch and ONE network.  The tile's activations live
//     in an LDS slab [32][260] f32, overwritten in place layer by layer; weights stream from L2 through a double-buffered LDS
//     chunk, read as they are (no packed image: the parameters change under every optimizer step).  Wave w produces output
//     columns [64w, 64w+64) = two 32x32 tiles of v_mfma_f32_32x32x2_f32.
//   backward-weights: dW_l = dZ_l^T H_{l-1} split-K over row ranges (slabs), 128x128 output tiles, 2x2 MFMA tiles per wave; bias
//     gradients ride along as column sums of the A fragments.
#pragma once

#include <algorithm>

#include "rlx_common.h"

namespace rlx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 32;     // rows per workgroup tile
constexpr int HID = 256;   // hidden width (fixed by the reference)
constexpr int XS = 260;    // LDS row stride of the activation slab (floats)
constexpr int KC = 32;     // k per weight chunk
constexpr int WS = 36;     // LDS row stride of a forward weight chunk [256][32]
constexpr int WT = 264;    // LDS row stride of a backward weight chunk [32][256]
constexpr int WBUF = HID * WS;  // floats per chunk buffer (>= 32 * WT)
// Xs | two chunk buffers | sOut [32][32] | sStat [32][2] f64
constexpr size_t LDS_BYTES = (size_t)(BM * XS + 2 * WBUF + 32 * 32 + 128) * sizeof(float);
static_assert((BM * XS + 2 * WBUF + 32 * 32) % 2 == 0, "sStat holds doubles");
static_assert(32 * WT <= WBUF, "backward chunk must fit the forward chunk buffer");
static_assert(BM * XS <= 2 * WBUF, "the chunk buffers double as the xhat slab of the LayerNorm backward");

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

__device__ __forceinline__ void zero_frag(f32x16 (&f)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) f[t][r] = 0.f;
}

// A 256-deep product is summed as eight 32-deep MFMA chains whose results are then added: the rounding error of a chain grows
// with its length, and one 128-step chain per output would leave these layers less exact than a blocked host GEMM's.
__device__ __forceinline__ void add_chunk(f32x16 (&acc)[2], const f32x16 (&part)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += part[t][r];
}

// acc[t] (t = 0,1) = Xs[0:32, 0:Kp] . Wg[64*wave + 32*t : +32, 0:K]^T     (all 256 threads must call)
//   Wg: global, row-major [256][ldw]; Kp = round_up(K, 8), Xs columns [K, Kp) are zero.  vec: ldw % 4 == 0 and Wg is
//   16-byte aligned.  Ends with a workgroup barrier.
__device__ __forceinline__ void tile_gemm(const float* __restrict__ Wg, int ldw, int K, int Kp, bool vec, const float* Xs,
                                          float* Ws, f32x16 (&acc)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, khalf = lane >> 5;
    const int ldrow = tid >> 3, ldc4 = (tid & 7) * 4;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float4 stage[8];
    auto gload = [&](int kc) {
        const int k = kc + ldc4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* p = Wg + (size_t)(ldrow + 32 * i) * ldw + k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (vec) {
                if (k < K) v = *reinterpret_cast<const float4*>(p);
            } else {
                if (k + 0 < K) v.x = p[0];
                if (k + 1 < K) v.y = p[1];
                if (k + 2 < K) v.z = p[2];
                if (k + 3 < K) v.w = p[3];
            }
            stage[i] = v;
        }
    };
    auto swrite = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<float4*>(buf + (ldrow + 32 * i) * WS + ldc4) = stage[i];
    };
    const int nchunks = (Kp + KC - 1) / KC;
    gload(0);
    swrite(Ws);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const float* cur = Ws + (c & 1) * WBUF;
        if (c + 1 < nchunks) gload((c + 1) * KC);
        const int kmax = min(KC, Kp - c * KC);
        const float* xa = Xs + lrow * XS + c * KC + 4 * khalf;
        const float* wb = cur + (wave * 64 + lrow) * WS + 4 * khalf;
        f32x16 part[2];  // this chunk's partial sums, added to the total once: see add_chunk
        zero_frag(part);
#pragma unroll 4
        for (int kk = 0; kk < kmax; kk += 8) {
            const float4 a = *reinterpret_cast<const float4*>(xa + kk);
            const float4 b0 = *reinterpret_cast<const float4*>(wb + kk);
            const float4 b1 = *reinterpret_cast<const float4*>(wb + 32 * WS + kk);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, part[1], 0, 0, 0);
        }
        add_chunk(acc, part);
        if (c + 1 < nchunks) swrite(Ws + ((c + 1) & 1) * WBUF);
        __syncthreads();
    }
}

// acc[t] = Xs[0:32, 0:256] . Wg[0:256, 64*wave + 32*t : +32]       (backward-data: dH = dZ . W, W row-major [256 out][256 in])
//   Wg 16-byte aligned.  Ends with a workgroup barrier.
__device__ __forceinline__ void tile_gemm_t(const float* __restrict__ Wg, const float* Xs, float* Ws, f32x16 (&acc)[2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, khalf = lane >> 5;
    const int ldrow = tid >> 6, ldc4 = (tid & 63) * 4;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float4 stage[8];
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 8; ++i) stage[i] = *reinterpret_cast<const float4*>(Wg + (size_t)(kc + ldrow + 4 * i) * HID + ldc4);
    };
    auto swrite = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<float4*>(buf + (ldrow + 4 * i) * WT + ldc4) = stage[i];
    };
    constexpr int nchunks = HID / KC;
    gload(0);
    swrite(Ws);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const float* cur = Ws + (c & 1) * WBUF;
        if (c + 1 < nchunks) gload((c + 1) * KC);
        const float* xa = Xs + lrow * XS + c * KC + 4 * khalf;
        const float* wb = cur + (4 * khalf) * WT + wave * 64 + lrow;
        f32x16 part[2];
        zero_frag(part);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 8) {
            const float4 a = *reinterpret_cast<const float4*>(xa + kk);
            const float* w = wb + kk * WT;
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[0], part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[32], part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[WT], part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[WT + 32], part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2 * WT], part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2 * WT + 32], part[1], 0, 0, 0);
            part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3 * WT], part[0], 0, 0, 0);
            part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3 * WT + 32], part[1], 0, 0, 0);
        }
        add_chunk(acc, part);
        if (c + 1 < nchunks) swrite(Ws + ((c + 1) & 1) * WBUF);
        __syncthreads();
    }
}

// C/D fragment of the 32x32 MFMA: register r of lane l holds (row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31)
__device__ __forceinline__ int frag_row(int r, int khalf) { return (r & 3) + 8 * (r >> 2) + 4 * khalf; }

// sum over the 8 consecutive lanes that share a row
__device__ __forceinline__ double sum8(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// out[row][o] (LDS, stride 32) = Xs[row][0:256] . W[o][0:256] + b[o], o < n_out <= 32      (no barrier)
//   Accumulated in f64 and rounded once: these few outputs per row (mean, raw log-std, Q) are what every loss is made of, and a
//   256-term f32 chain would leave them with several ulps of their partial sums; 256 x n_out f64 FMAs per row cost nothing
//   next to the three 256 x 256 layers.
__device__ __forceinline__ void head_dots(const float* Xs, const float* __restrict__ W, const float* __restrict__ b, int n_out,
                                          float* sOut) {
    for (int idx = threadIdx.x; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        const float* xr = Xs + row * XS;
        const float* wr = W + (size_t)o * HID;
        double s = 0.0;
#pragma unroll 8
        for (int j = 0; j < HID; j += 4) {
            const float4 x = *reinterpret_cast<const float4*>(xr + j);
            const float4 w = *reinterpret_cast<const float4*>(wr + j);
            s = fma((double)x.x, (double)w.x, s);
            s = fma((double)x.y, (double)w.y, s);
            s = fma((double)x.z, (double)w.z, s);
            s = fma((double)x.w, (double)w.w, s);
        }
        sOut[row * 32 + o] = (float)(s + (double)b[o]);
    }
}

// thread j: s[row] = sum_o sOut[row][o] * W[o][j]  -> fn(row, j, s)        (n_out <= 32)
template <typename F>
__device__ __forceinline__ void head_back(const float* sOut, const float* __restrict__ W, int n_out, F fn) {
    const int j = threadIdx.x;
    float w[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) w[o] = o < n_out ? W[(size_t)o * HID + j] : 0.f;
    for (int row = 0; row < BM; ++row) {
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < 32; ++o)
            if (o < n_out) s = fmaf(sOut[row * 32 + o], w[o], s);
        fn(row, j, s);
    }
}

// ===================================================================================================
// backward-weights: slab s of dW = A^T B and db = column sums of A, per job
//   grid = (slabs, 4 output tiles of 128x128, jobs)
// ===================================================================================================
constexpr int MAX_DW_JOBS = 6;
struct DwJob {
    const float* A;    // [M][256]  gradient at the layer's output
    const float* B0;   // [M][K0]   the layer's input ...
    const float* B1;   // [M][K1]   ... and its second part (the Q first layer's actions), or nullptr
    int K0, K1;
    long long off_w, off_b;
};
struct DwArgs {
    DwJob job[MAX_DW_JOBS];
    long long M, n_params;
    int rows_per_slab;  // multiple of 32
    float* grads;       // [slabs][n_params]
};

__global__ __launch_bounds__(256) void mlp_dw_kernel(DwArgs a) {
    __shared__ __align__(16) float As[2][32][128];
    __shared__ __align__(16) float Bs[2][32][128];
    const int s = blockIdx.x, tile = blockIdx.y;
    const DwJob& jb = a.job[blockIdx.z];
    const long long M = a.M;
    const int K0 = jb.K0, Kin = jb.K0 + jb.K1;
    const int i0 = (tile >> 1) * 128, j0 = (tile & 1) * 128;
    if (j0 >= Kin) return;
    const float* A = jb.A;
    const bool vecB = jb.B1 == nullptr && (K0 % 4) == 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, khalf = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const long long r_begin = (long long)s * a.rows_per_slab;
    const long long r_end = min(M, r_begin + a.rows_per_slab);
    const int nchunks = r_end > r_begin ? (int)((r_end - r_begin + 31) / 32) : 0;

    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    float bsum[2] = {0.f, 0.f};

    const int ldr = tid >> 5, ldc4 = (tid & 31) * 4;
    float4 sa[4], sb[4];
    auto bval = [&](long long row, int col) {
        if (col < K0) return jb.B0[(size_t)row * K0 + col];
        if (col < Kin) return jb.B1[(size_t)row * jb.K1 + (col - K0)];
        return 0.f;
    };
    auto gload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long row = r_begin + (long long)c * 32 + ldr + 8 * i;
            const bool ok = row < r_end;
            sa[i] = ok ? *reinterpret_cast<const float4*>(A + (size_t)row * HID + i0 + ldc4) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const int col = j0 + ldc4;
                if (vecB) {
                    if (col < Kin) v = *reinterpret_cast<const float4*>(jb.B0 + (size_t)row * K0 + col);
                } else {
                    v = make_float4(bval(row, col), bval(row, col + 1), bval(row, col + 2), bval(row, col + 3));
                }
            }
            sb[i] = v;
        }
    };
    auto swrite = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4*>(&As[buf][ldr + 8 * i][ldc4]) = sa[i];
            *reinterpret_cast<float4*>(&Bs[buf][ldr + 8 * i][ldc4]) = sb[i];
        }
    };
    if (nchunks > 0) {
        gload(0);
        swrite(0);
    }
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunks) gload(c + 1);
#pragma unroll 4
        for (int kp = 0; kp < 16; ++kp) {
            const int k = 2 * kp + khalf;
            const float a0 = As[cur][k][wi * 64 + lrow], a1 = As[cur][k][wi * 64 + 32 + lrow];
            const float b0 = Bs[cur][k][wj * 64 + lrow], b1 = Bs[cur][k][wj * 64 + 32 + lrow];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            bsum[0] += a0;
            bsum[1] += a1;
        }
        if (c + 1 < nchunks) swrite(cur ^ 1);
        __syncthreads();
    }
    float* slab = a.grads + (size_t)s * a.n_params;
    float* dW = slab + jb.off_w;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = j0 + wj * 64 + u * 32 + lrow;
            if (col < Kin) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i0 + wi * 64 + t * 32 + frag_row(r, khalf);
                    dW[(size_t)row * Kin + col] = acc[t][u][r];
                }
            }
        }
    if (j0 == 0 && wj == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float tot = bsum[t] + __shfl_xor(bsum[t], 32, 64);
            if (khalf == 0) slab[jb.off_b + i0 + wi * 64 + t * 32 + lrow] = tot;
        }
    }
}

// ---- host side ----
bool in_range(int64_t off, int64_t len, int64_t n) { return off >= 0 && len >= 0 && off + len <= n; }

// once per kernel and process (not a stream operation)
template <typename K>
int set_lds(K kern) {
    static thread_local const void* done[8] = {};
    const void* key = reinterpret_cast<const void*>(kern);
    for (const void* d : done)
        if (d == key) return RLX_OK;
    RLX_HIP_CHECK(hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    for (auto& d : done)
        if (d == nullptr) { d = key; break; }
    return RLX_OK;
}

int bwd_slabs(int64_t m) { return (int)std::max<int64_t>(1, std::min<int64_t>(64, (m + 511) / 512)); }

}  // namespace
}  // namespace rlx
