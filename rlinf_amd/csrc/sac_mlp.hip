// sac_mlp.hip -- the model calls of the SAC (Q-head) variant of the MLP policy, gfx950, f32 only.
//
// Replaces MLPPolicy(add_q_head=True) (rlinf/models/embodiment/mlp_policy/mlp_policy.py): sac_forward :179-200 and
// _sample_actions / _generate_actions with final_tanh :238-293 (actor); sac_q_forward :322-323 -> MultiQHead / QHead
// (rlinf/models/embodiment/modules/q_head.py:22-160) over make_mlp's Linear -> LayerNorm -> tanh stack
// (modules/utils.py:38-50); Normal.rsample / log_prob; and autograd's backward through all of it.
//
// Work decomposition: the tile scheme of mlp_policy.hip; the tile GEMMs, head helpers and the weight-gradient kernel are in
// rlx_mlp_tile.h, shared with iql_mlp.hip.
//   forward / backward-data: one workgroup (4 waves) owns a 32-row tile of the batch and ONE network (actor; Q: blockIdx.y =
//     head).  The tile's activations live in an LDS slab [32][260] f32, overwritten in place layer by layer; weights stream
//     from L2 through a double-buffered LDS chunk.  Wave w produces output columns [64w, 64w+64) = two 32x32 tiles of
//     v_mfma_f32_32x32x2_f32.  Unlike mlp_policy.hip there is NO packed weight image: the parameters change under every
//     optimizer step and every soft update, so the kernels read them as they are.  The forward chunk is [256 out][32 k] read
//     with one b128 per operand; backward-data needs W^T, and streams the SAME row-major weights as a chunk [32 k][256 in]
//     whose B operands are b32 reads (row stride 264: the two k-halves of a wave land 32 banks apart).  The Q first layer
//     reads states and actions side by side (K = D + A' need not be a multiple of 4: scalar chunk loads, zero-padded to 8).
//   LayerNorm: a row's 256 pre-activations span the four waves' column ranges, so the row statistics (mean, then the centred
//     second moment -- two passes, as torch's CPU kernel) are a cross-wave reduction through the LDS slab: 8 threads per row,
//     32 columns each, combined with wave shuffles.  Backward reduces sum(g) and sum(g * xhat) the same way.
//   backward-weights: dW_l = dZ_l^T H_{l-1} split-K over row ranges (slabs), 128x128 output tiles, 2x2 MFMA tiles per wave;
//     bias gradients ride along as column sums of the A fragments; LayerNorm affine and head gradients are column loops.
//     Slabs are summed by rlx_sum_slabs.
// Exactness: the MFMA is an exact-f32 fmaf chain; results differ from the reference's f32 run by summation order and by
// the f32 roundings between the layers.  What is cheap next to the 256 x 256 layers runs in f64 and rounds once: tanh, the
// LayerNorm statistics and normalisation, the few head outputs per row, the actor's per-element distribution epilogue.

#include <algorithm>

#include "rlx_mlp_tile.h"  // tile_gemm, tile_gemm_t, the head helpers, mlp_dw_kernel, set_lds, bwd_slabs

namespace rlx {
namespace {

constexpr int MAX_D = 64, MAX_A = 16;
constexpr float LN_EPS = 1e-5f;

// ===================================================================================================
// actor
// ===================================================================================================
struct ActorFwdArgs {
    const float* params;
    rlx_sac_actor_layout lay;
    const float* states;
    const float* eps;   // or nullptr: raw = mean
    long long M;
    float scale, bias;
    float* action;
    float* logprob;
    float* acts;        // [3][M][256] or nullptr
    float* aux;         // [2][M][A] or nullptr
};

__device__ __forceinline__ void tanh_epilogue(const f32x16 (&acc)[2], const float* __restrict__ bias, float* Xs,
                                              float* __restrict__ save, long long m0, long long M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = wave * 64 + t * 32 + lrow;
        const float b = bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = frag_row(r, khalf);
            const float h = (float)tanh((double)acc[t][r] + (double)b);  // rounds once: tanhf alone is 1-2 ulp off
            Xs[row * XS + col] = h;
            if (save != nullptr && m0 + row < M) save[(size_t)(m0 + row) * HID + col] = h;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void sac_actor_fwd_kernel(ActorFwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* sOut = Ws + 2 * WBUF;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_sac_actor_layout& lay = a.lay;
    const int D = lay.obs_dim, Dp = round_up(D, 8), A = lay.act_dim, tid = threadIdx.x;
    for (int i = tid; i < BM * Dp; i += 256) {
        const int r = i / Dp, c = i % Dp;
        Xs[r * XS + c] = (c < D && m0 + r < M) ? a.states[(size_t)(m0 + r) * D + c] : 0.f;
    }
    f32x16 acc[2];
    const size_t MH = (size_t)M * HID;
    tile_gemm(a.params + lay.off_w[0], D, D, Dp, (D % 4) == 0 && (lay.off_w[0] % 4) == 0, Xs, Ws, acc);
    tanh_epilogue(acc, a.params + lay.off_b[0], Xs, a.acts, m0, M);
    tile_gemm(a.params + lay.off_w[1], HID, HID, HID, true, Xs, Ws, acc);
    tanh_epilogue(acc, a.params + lay.off_b[1], Xs, a.acts ? a.acts + MH : nullptr, m0, M);
    tile_gemm(a.params + lay.off_w[2], HID, HID, HID, true, Xs, Ws, acc);
    tanh_epilogue(acc, a.params + lay.off_b[2], Xs, a.acts ? a.acts + 2 * MH : nullptr, m0, M);

    head_dots(Xs, a.params + lay.off_wh, a.params + lay.off_bh, 2 * A, sOut);  // [mean | raw log-std]
    __syncthreads();
    const float lo = lay.logstd_lo, half_range = 0.5f * (lay.logstd_hi - lay.logstd_lo);
    for (int idx = tid; idx < BM * A; idx += 256) {
        const int row = idx / A, o = idx % A;
        if (m0 + row >= M) continue;
        const size_t g = (size_t)(m0 + row) * A + o;
        // a handful of elements per row: the distribution epilogue runs in f64 and rounds once.  Its terms are O(1..5) and
        // cancel (the log-prob of a near-deterministic policy is a small difference of large terms), so f32 steps would each
        // leave an error of an ulp of the LARGEST term in the result.
        const double mean = sOut[row * 32 + o];
        const double t = tanh((double)sOut[row * 32 + A + o]);
        const double logstd = (double)lo + (double)half_range * (t + 1.0);
        const double stdv = exp(logstd);
        const double e = a.eps ? (double)a.eps[g] : 0.0;
        const double raw = mean + e * stdv;  // Normal.rsample: loc + eps * scale
        const double an = tanh(raw);
        // Normal.log_prob: -((x - loc)**2) / (2*var) - log(scale) - log(sqrt(2*pi)); then the tanh-squash correction
        const double lp = -0.5 * e * e - logstd - 0.91893853320467274178 - log((double)a.scale * (1.0 - an * an) + 1e-6);
        a.action[g] = (float)(an * (double)a.scale + (double)a.bias);
        a.logprob[g] = (float)lp;
        if (a.aux) {
            a.aux[g] = (float)t;
            a.aux[(size_t)M * A + g] = (float)an;
        }
    }
}

struct ActorBwdArgs {
    const float* params;
    rlx_sac_actor_layout lay;
    const float* eps;        // or nullptr
    const float* acts;       // [3][M][256]
    const float* aux;        // [2][M][A]
    const float* d_action;   // [M][A] or nullptr
    const float* d_logprob;  // [M][A] or nullptr
    long long M;
    float scale;
    float* dz;               // [3][M][256]
    float* dout;             // [M][2A]: d/d mean | d/d raw log-std
};

__device__ __forceinline__ void tanh_bwd_epilogue(const f32x16 (&acc)[2], const float* __restrict__ hsaved, float* Xs,
                                                  float* __restrict__ dz_out, long long m0, long long M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = wave * 64 + t * 32 + lrow;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = frag_row(r, khalf);
            float dz = 0.f;
            if (m0 + row < M) {
                const float h = hsaved[(size_t)(m0 + row) * HID + col];
                dz = acc[t][r] * (1.f - h * h);
                dz_out[(size_t)(m0 + row) * HID + col] = dz;
            }
            Xs[row * XS + col] = dz;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void sac_actor_bwd_dz_kernel(ActorBwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* sOut = Ws + 2 * WBUF;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_sac_actor_layout& lay = a.lay;
    const int A = lay.act_dim, tid = threadIdx.x;
    const size_t MH = (size_t)M * HID;
    const float lo = lay.logstd_lo, half_range = 0.5f * (lay.logstd_hi - lay.logstd_lo);
    for (int idx = tid; idx < BM * A; idx += 256) {
        const int row = idx / A, o = idx % A;
        float g_mean = 0.f, g_rls = 0.f;
        if (m0 + row < M) {
            const size_t g = (size_t)(m0 + row) * A + o;
            const float t = a.aux[g], an = a.aux[(size_t)M * A + g];
            const float stdv = expf(lo + half_range * (t + 1.f));
            const float e = a.eps ? a.eps[g] : 0.f;
            const float dA = a.d_action ? a.d_action[g] : 0.f, dL = a.d_logprob ? a.d_logprob[g] : 0.f;
            const float om = 1.f - an * an;
            // raw = mean + std * eps: the Normal.log_prob term is -eps^2/2 - logstd - const along the rsample path, so
            // d logprob / d mean is the squash correction alone and d logprob / d logstd adds -1
            const float g_raw = dA * a.scale * om + dL * (2.f * a.scale * an * om / (a.scale * om + 1e-6f));
            g_mean = g_raw;
            g_rls = (g_raw * stdv * e - dL) * half_range * (1.f - t * t);
            a.dout[(size_t)(m0 + row) * 2 * A + o] = g_mean;
            a.dout[(size_t)(m0 + row) * 2 * A + A + o] = g_rls;
        }
        sOut[row * 32 + o] = g_mean;
        sOut[row * 32 + A + o] = g_rls;
    }
    __syncthreads();
    {
        const float* h3 = a.acts + 2 * MH;
        float* dz3 = a.dz + 2 * MH;
        head_back(sOut, a.params + lay.off_wh, 2 * A, [&](int row, int j, float s) {
            float dzv = 0.f;
            if (m0 + row < M) {
                const float h = h3[(size_t)(m0 + row) * HID + j];
                dzv = s * (1.f - h * h);
                dz3[(size_t)(m0 + row) * HID + j] = dzv;
            }
            Xs[row * XS + j] = dzv;
        });
    }
    __syncthreads();
    f32x16 acc[2];
    tile_gemm_t(a.params + lay.off_w[2], Xs, Ws, acc);
    tanh_bwd_epilogue(acc, a.acts + MH, Xs, a.dz + MH, m0, M);
    tile_gemm_t(a.params + lay.off_w[1], Xs, Ws, acc);
    tanh_bwd_epilogue(acc, a.acts, Xs, a.dz, m0, M);
}

// ===================================================================================================
// Q ensemble
// ===================================================================================================
struct QFwdArgs {
    const float* params;
    rlx_sac_q_layout lay;
    const float* states;
    const float* actions;
    long long M;
    float* q;      // [M][2*out]
    float* acts;   // [2][3][2][M][256] or nullptr
    float* rstd;   // [2][3][M] or nullptr
};

// z = acc + bias -> LayerNorm over the row -> tanh, in place in the slab [+ saves h, xhat, rstd]
__device__ __forceinline__ void ln_tanh_epilogue(const f32x16 (&acc)[2], const float* __restrict__ bias,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* Xs,
                                                 double* sStat, float* __restrict__ save_h, float* __restrict__ save_xh,
                                                 float* __restrict__ save_rstd, long long m0, long long M) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = wave * 64 + t * 32 + lrow;
        const float b = bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) Xs[frag_row(r, khalf) * XS + col] = acc[t][r] + b;
    }
    __syncthreads();
    {
        const int row = tid >> 3, part = tid & 7;
        const float* xr = Xs + row * XS + part * 32;
        double s = 0.0;  // the row statistics and the normalisation run in f64 (a few thousand elements per tile) and round once
#pragma unroll
        for (int j = 0; j < 32; ++j) s += (double)xr[j];
        const double mean = sum8(s) * (1.0 / HID);
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const double d = (double)xr[j] - mean;
            v = fma(d, d, v);
        }
        const double rstd = 1.0 / sqrt(sum8(v) * (1.0 / HID) + (double)LN_EPS);
        if (part == 0) {
            sStat[2 * row] = mean;
            sStat[2 * row + 1] = rstd;
            if (save_rstd != nullptr && m0 + row < M) save_rstd[m0 + row] = (float)rstd;
        }
    }
    __syncthreads();
    {
        const int j = tid;
        const float g = gamma[j], be = beta[j];
        for (int row = 0; row < BM; ++row) {
            const double xh = ((double)Xs[row * XS + j] - sStat[2 * row]) * sStat[2 * row + 1];
            const float h = (float)tanh(xh * (double)g + (double)be);
            Xs[row * XS + j] = h;
            if (save_h != nullptr && m0 + row < M) {
                save_h[(size_t)(m0 + row) * HID + j] = h;
                save_xh[(size_t)(m0 + row) * HID + j] = (float)xh;
            }
        }
    }
    __syncthreads();
}

// the slab's first-layer input: cat(states, actions) rows, zero-padded to Kp columns and past M
__device__ __forceinline__ void load_state_action(float* Xs, const float* __restrict__ states, const float* __restrict__ actions,
                                                  int D, int A, int Kp, long long m0, long long M) {
    for (int i = threadIdx.x; i < BM * Kp; i += 256) {
        const int r = i / Kp, c = i % Kp;
        float v = 0.f;
        if (m0 + r < M) {
            if (c < D) v = states[(size_t)(m0 + r) * D + c];
            else if (c < D + A) v = actions[(size_t)(m0 + r) * A + (c - D)];
        }
        Xs[r * XS + c] = v;
    }
}

__global__ __launch_bounds__(256) void sac_q_fwd_kernel(QFwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* sOut = Ws + 2 * WBUF;
    double* sStat = reinterpret_cast<double*>(sOut + 32 * 32);
    const int y = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_sac_q_layout& lay = a.lay;
    const int D = lay.obs_dim, A = lay.act_dim, K = D + A, Kp = round_up(K, 8), n_out = lay.out_dim, tid = threadIdx.x;
    const size_t MH = (size_t)M * HID;
    load_state_action(Xs, a.states, a.actions, D, A, Kp, m0, M);
    f32x16 acc[2];
    for (int l = 0; l < 3; ++l) {
        if (l == 0) tile_gemm(a.params + lay.off_w[y][0], K, K, Kp, (K % 4) == 0 && (lay.off_w[y][0] % 4) == 0, Xs, Ws, acc);
        else tile_gemm(a.params + lay.off_w[y][l], HID, HID, HID, true, Xs, Ws, acc);
        float* sh = a.acts ? a.acts + (size_t)((y * 3 + l) * 2) * MH : nullptr;
        ln_tanh_epilogue(acc, a.params + lay.off_b[y][l], a.params + lay.off_g[y][l], a.params + lay.off_beta[y][l], Xs, sStat, sh,
                         sh ? sh + MH : nullptr, a.rstd ? a.rstd + (size_t)(y * 3 + l) * M : nullptr, m0, M);
    }
    head_dots(Xs, a.params + lay.off_w[y][3], a.params + lay.off_b[y][3], n_out, sOut);
    __syncthreads();
    for (int idx = tid; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        if (m0 + row < M) a.q[(size_t)(m0 + row) * 2 * n_out + y * n_out + o] = sOut[row * 32 + o];
    }
}

struct QBwdArgs {
    const float* params;
    rlx_sac_q_layout lay;
    const float* acts;   // [2][3][2][M][256]
    const float* rstd;   // [2][3][M]
    const float* d_q;    // [M][2*out]
    long long M;
    float* dz;           // [2][3][M][256]  gradient at the Linear outputs
    float* dy;           // [2][3][M][256]  gradient at the LayerNorm outputs (for its affine parameters)
    float* d_actions;    // [M][A], zeroed by the caller; or nullptr
};

// Xs holds g = dy * gamma, Xh the xhat slab (both zero past M): Xs <- dz = rstd * (g - mean(g) - xhat * mean(g * xhat))
__device__ __forceinline__ void ln_bwd_finish(float* Xs, const float* Xh, double* sStat, const float* __restrict__ rstd,
                                              float* __restrict__ dz_out, long long m0, long long M) {
    const int tid = threadIdx.x;
    __syncthreads();
    {
        const int row = tid >> 3, part = tid & 7;
        const float* gr = Xs + row * XS + part * 32;
        const float* xr = Xh + row * XS + part * 32;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            s1 += (double)gr[j];
            s2 = fma((double)gr[j], (double)xr[j], s2);
        }
        s1 = sum8(s1), s2 = sum8(s2);
        if (part == 0) {
            sStat[2 * row] = s1 * (1.0 / HID);
            sStat[2 * row + 1] = s2 * (1.0 / HID);
        }
    }
    __syncthreads();
    {
        const int j = tid;
        for (int row = 0; row < BM; ++row) {
            float dz = 0.f;
            if (m0 + row < M) {
                dz = (float)((double)rstd[m0 + row] *
                             ((double)Xs[row * XS + j] - sStat[2 * row] - (double)Xh[row * XS + j] * sStat[2 * row + 1]));
                dz_out[(size_t)(m0 + row) * HID + j] = dz;
            }
            Xs[row * XS + j] = dz;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void sac_q_bwd_dz_kernel(QBwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* Xh = Ws;  // the chunk buffers are idle between two products
    float* sOut = Ws + 2 * WBUF;
    double* sStat = reinterpret_cast<double*>(sOut + 32 * 32);
    const int y = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_sac_q_layout& lay = a.lay;
    const int D = lay.obs_dim, A = lay.act_dim, n_out = lay.out_dim, tid = threadIdx.x;
    const size_t MH = (size_t)M * HID;
    auto H = [&](int l) { return a.acts + (size_t)((y * 3 + l) * 2) * MH; };
    auto slot = [&](float* base, int l) { return base + (size_t)(y * 3 + l) * MH; };

    for (int idx = tid; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        sOut[row * 32 + o] = m0 + row < M ? a.d_q[(size_t)(m0 + row) * 2 * n_out + y * n_out + o] : 0.f;
    }
    __syncthreads();
    {
        const float* h3 = H(2);
        const float* xh3 = h3 + MH;
        float* dy3 = slot(a.dy, 2);
        const float gam = a.params[lay.off_g[y][2] + tid];
        head_back(sOut, a.params + lay.off_w[y][3], n_out, [&](int row, int j, float s) {
            float g = 0.f, xh = 0.f;
            if (m0 + row < M) {
                const size_t at = (size_t)(m0 + row) * HID + j;
                const float h = h3[at];
                const float dyv = s * (1.f - h * h);
                dy3[at] = dyv;
                g = dyv * gam;
                xh = xh3[at];
            }
            Xs[row * XS + j] = g;
            Xh[row * XS + j] = xh;
        });
    }
    ln_bwd_finish(Xs, Xh, sStat, a.rstd + (size_t)(y * 3 + 2) * M, slot(a.dz, 2), m0, M);
    f32x16 acc[2];
    for (int l = 1; l >= 0; --l) {
        tile_gemm_t(a.params + lay.off_w[y][l + 1], Xs, Ws, acc);  // dH_l = dZ_{l+1} . W_{l+1}
        const int lane = tid & 63, wave = tid >> 6, lrow = lane & 31, khalf = lane >> 5;
        const float* hl = H(l);
        const float* xhl = hl + MH;
        float* dyl = slot(a.dy, l);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int col = wave * 64 + t * 32 + lrow;
            const float gam = a.params[lay.off_g[y][l] + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = frag_row(r, khalf);
                float g = 0.f, xh = 0.f;
                if (m0 + row < M) {
                    const size_t at = (size_t)(m0 + row) * HID + col;
                    const float h = hl[at];
                    const float dyv = acc[t][r] * (1.f - h * h);
                    dyl[at] = dyv;
                    g = dyv * gam;
                    xh = xhl[at];
                }
                Xs[row * XS + col] = g;
                Xh[row * XS + col] = xh;
            }
        }
        ln_bwd_finish(Xs, Xh, sStat, a.rstd + (size_t)(y * 3 + l) * M, slot(a.dz, l), m0, M);
    }
    if (a.d_actions != nullptr) {  // d cat(states, actions) = dZ_1 . W_1, the action columns only; the two heads add up
        const int K = D + A;
        const float* W1 = a.params + lay.off_w[y][0];
        for (int idx = tid; idx < BM * A; idx += 256) {
            const int row = idx / A, c = idx % A;
            if (m0 + row >= M) continue;
            float s = 0.f;
            for (int k = 0; k < HID; ++k) s = fmaf(Xs[row * XS + k], W1[(size_t)k * K + D + c], s);
            atomicAdd(a.d_actions + (size_t)(m0 + row) * A + c, s);  // 0 + a + b: the order of the two heads does not matter
        }
    }
}

// Column jobs of slab s (thread = hidden column j).  grid = (slabs, jobs)
//   head: dW[o][j] = sum_rows dout[row][o] * h[row][j], db[o] = sum_rows dout[row][o]        (n_out > 0)
//   LayerNorm affine: dgamma[j] = sum_rows dy[row][j] * xhat[row][j], dbeta[j] = sum_rows dy  (n_out == 0: P = dy, Q = xhat)
constexpr int MAX_COL_JOBS = 8;
struct ColJob {
    const float* P;
    const float* Q;
    int n_out, ld_p, col0;   // head: dout[row][o] = P[row * ld_p + col0 + o]
    long long off_1, off_2;  // head: weight, bias; LayerNorm: gamma, beta
};
struct ColArgs {
    ColJob job[MAX_COL_JOBS];
    long long M, n_params;
    int rows_per_slab;
    float* grads;
};

__global__ __launch_bounds__(256) void sac_col_kernel(ColArgs a) {
    const int s = blockIdx.x, j = threadIdx.x;
    const ColJob& jb = a.job[blockIdx.y];
    const long long r_begin = (long long)s * a.rows_per_slab, r_end = min(a.M, r_begin + a.rows_per_slab);
    float* slab = a.grads + (size_t)s * a.n_params;
    if (jb.n_out == 0) {
        float sg = 0.f, sb = 0.f;
        for (long long row = r_begin; row < r_end; ++row) {
            const float dy = jb.P[(size_t)row * HID + j];
            sg = fmaf(dy, jb.Q[(size_t)row * HID + j], sg);
            sb += dy;
        }
        slab[jb.off_1 + j] = sg;
        slab[jb.off_2 + j] = sb;
        return;
    }
    const int n_out = jb.n_out;
    for (int o0 = 0; o0 < n_out; o0 += 8) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int no = min(8, n_out - o0);
        for (long long row = r_begin; row < r_end; ++row) {
            const float h = jb.Q[(size_t)row * HID + j];
            const float* d = jb.P + (size_t)row * jb.ld_p + jb.col0 + o0;
#pragma unroll
            for (int o = 0; o < 8; ++o)
                if (o < no) acc[o] = fmaf(d[o], h, acc[o]);
        }
        for (int o = 0; o < no; ++o) slab[jb.off_1 + (size_t)(o0 + o) * HID + j] = acc[o];
    }
    if (j < n_out) {
        float sb = 0.f;
        for (long long row = r_begin; row < r_end; ++row) sb += jb.P[(size_t)row * jb.ld_p + jb.col0 + j];
        slab[jb.off_2 + j] = sb;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

int check_dims(const char* who, int hidden, int obs_dim, int act_dim) {
    RLX_REQUIRE(hidden == HID, "%s: hidden=%d is not supported (the reference's MLP policy is 256 wide)", who, hidden);
    RLX_REQUIRE(obs_dim >= 1 && obs_dim <= MAX_D, "%s: obs_dim=%d out of range [1,%d]", who, obs_dim, MAX_D);
    RLX_REQUIRE(act_dim >= 1 && act_dim <= MAX_A, "%s: act_dim=%d out of range [1,%d]", who, act_dim, MAX_A);
    return RLX_OK;
}

int check_actor(const rlx_sac_actor_layout* lay, const char* who) {
    RLX_REQUIRE(lay != nullptr, "%s: NULL layout", who);
    if (int rc = check_dims(who, lay->hidden, lay->obs_dim, lay->act_dim)) return rc;
    const int64_t n = lay->n_params;
    for (int l = 0; l < 3; ++l) {
        RLX_REQUIRE(in_range(lay->off_w[l], (int64_t)HID * (l == 0 ? lay->obs_dim : HID), n) && in_range(lay->off_b[l], HID, n),
                    "%s: offset of backbone layer %d out of range", who, l);
        RLX_REQUIRE(l == 0 || lay->off_w[l] % 4 == 0, "%s: offsets of the 256-wide weights must be multiples of 4", who);
    }
    RLX_REQUIRE(in_range(lay->off_wh, (int64_t)2 * lay->act_dim * HID, n) && in_range(lay->off_bh, 2 * lay->act_dim, n),
                "%s: head offset out of range", who);
    RLX_REQUIRE(lay->off_wh % 4 == 0, "%s: offsets of the 256-wide weights must be multiples of 4", who);
    return RLX_OK;
}

int check_q(const rlx_sac_q_layout* lay, const char* who) {
    RLX_REQUIRE(lay != nullptr, "%s: NULL layout", who);
    if (int rc = check_dims(who, lay->hidden, lay->obs_dim, lay->act_dim)) return rc;
    RLX_REQUIRE(lay->out_dim >= 1 && lay->out_dim <= MAX_A, "%s: out_dim=%d out of range [1,%d]", who, lay->out_dim, MAX_A);
    const int64_t n = lay->n_params;
    for (int y = 0; y < 2; ++y)
        for (int l = 0; l < 4; ++l) {
            const int64_t rows = l == 3 ? lay->out_dim : HID, cols = l == 0 ? lay->obs_dim + lay->act_dim : HID;
            RLX_REQUIRE(in_range(lay->off_w[y][l], rows * cols, n) && in_range(lay->off_b[y][l], rows, n),
                        "%s: offset of head %d layer %d out of range", who, y, l);
            RLX_REQUIRE(l == 0 || lay->off_w[y][l] % 4 == 0, "%s: offsets of the 256-wide weights must be multiples of 4", who);
            RLX_REQUIRE(l == 3 || (in_range(lay->off_g[y][l], HID, n) && in_range(lay->off_beta[y][l], HID, n)),
                        "%s: LayerNorm offset of head %d layer %d out of range", who, y, l);
        }
    return RLX_OK;
}


}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_sac_actor_fwd(const float* params, const rlx_sac_actor_layout* lay, const float* states, const float* eps,
                                 int64_t m, float action_scale, float action_bias, float* action, float* logprob, float* acts,
                                 float* aux, rlx_stream_t stream) {
    if (int rc = check_actor(lay, "rlx_sac_actor_fwd")) return rc;
    RLX_REQUIRE(m >= 0, "rlx_sac_actor_fwd: negative batch");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(params && states && action && logprob, "rlx_sac_actor_fwd: NULL argument");
    RLX_REQUIRE((acts == nullptr) == (aux == nullptr), "rlx_sac_actor_fwd: acts and aux go together (both NULL: no-grad form)");
    if (int rc = set_lds(sac_actor_fwd_kernel)) return rc;
    ActorFwdArgs a{};
    a.params = params; a.lay = *lay; a.states = states; a.eps = eps; a.M = m; a.scale = action_scale; a.bias = action_bias;
    a.action = action; a.logprob = logprob; a.acts = acts; a.aux = aux;
    hipLaunchKernelGGL(sac_actor_fwd_kernel, dim3(ceil_div(m, BM)), dim3(256), LDS_BYTES, static_cast<hipStream_t>(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_sac_actor_bwd_slabs(int64_t m) { return bwd_slabs(m); }

extern "C" size_t rlx_sac_actor_bwd_workspace_bytes(const rlx_sac_actor_layout* lay, int64_t m) {
    if (!lay || m <= 0) return 16;
    return ((size_t)3 * m * HID + 2 * (size_t)m * lay->act_dim) * sizeof(float);
}

extern "C" int rlx_sac_actor_bwd(const float* params, const rlx_sac_actor_layout* lay, const float* states, const float* eps,
                                 const float* acts, const float* aux, const float* d_action, const float* d_logprob, int64_t m,
                                 float action_scale, float* grads, int slabs, void* workspace, size_t workspace_bytes,
                                 rlx_stream_t stream) {
    if (int rc = check_actor(lay, "rlx_sac_actor_bwd")) return rc;
    RLX_REQUIRE(m >= 1, "rlx_sac_actor_bwd: empty batch");
    RLX_REQUIRE(slabs >= 1, "rlx_sac_actor_bwd: slabs=%d", slabs);
    RLX_REQUIRE(params && states && acts && aux && grads && workspace, "rlx_sac_actor_bwd: NULL argument");
    if (workspace_bytes < rlx_sac_actor_bwd_workspace_bytes(lay, m)) {
        set_error("rlx_sac_actor_bwd: workspace %zu < %zu bytes", workspace_bytes, rlx_sac_actor_bwd_workspace_bytes(lay, m));
        return RLX_ENOSPC;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t MH = (size_t)m * HID;
    const int A = lay->act_dim;
    float* dz = static_cast<float*>(workspace);
    float* dout = dz + 3 * MH;
    if (int rc = set_lds(sac_actor_bwd_dz_kernel)) return rc;
    ActorBwdArgs b{};
    b.params = params; b.lay = *lay; b.eps = eps; b.acts = acts; b.aux = aux; b.d_action = d_action; b.d_logprob = d_logprob;
    b.M = m; b.scale = action_scale; b.dz = dz; b.dout = dout;
    hipLaunchKernelGGL(sac_actor_bwd_dz_kernel, dim3(ceil_div(m, BM)), dim3(256), LDS_BYTES, s, b);
    RLX_LAUNCH_CHECK();
    const int rows_per_slab = round_up((int)((m + slabs - 1) / slabs), 32);
    DwArgs d{};
    d.M = m; d.n_params = lay->n_params; d.rows_per_slab = rows_per_slab; d.grads = grads;
    for (int l = 0; l < 3; ++l)
        d.job[l] = DwJob{dz + l * MH, l == 0 ? states : acts + (l - 1) * MH, nullptr, l == 0 ? lay->obs_dim : HID, 0,
                         lay->off_w[l], lay->off_b[l]};
    hipLaunchKernelGGL(mlp_dw_kernel, dim3(slabs, 4, 3), dim3(256), 0, s, d);
    RLX_LAUNCH_CHECK();
    ColArgs c{};
    c.M = m; c.n_params = lay->n_params; c.rows_per_slab = rows_per_slab; c.grads = grads;
    c.job[0] = ColJob{dout, acts + 2 * MH, 2 * A, 2 * A, 0, lay->off_wh, lay->off_bh};
    hipLaunchKernelGGL(sac_col_kernel, dim3(slabs, 1), dim3(256), 0, s, c);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_sac_q_fwd(const float* params, const rlx_sac_q_layout* lay, const float* states, const float* actions,
                             int64_t m, float* q, float* acts, float* rstd, rlx_stream_t stream) {
    if (int rc = check_q(lay, "rlx_sac_q_fwd")) return rc;
    RLX_REQUIRE(m >= 0, "rlx_sac_q_fwd: negative batch");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(params && states && actions && q, "rlx_sac_q_fwd: NULL argument");
    RLX_REQUIRE((acts == nullptr) == (rstd == nullptr), "rlx_sac_q_fwd: acts and rstd go together (both NULL: no-grad form)");
    if (int rc = set_lds(sac_q_fwd_kernel)) return rc;
    QFwdArgs a{};
    a.params = params; a.lay = *lay; a.states = states; a.actions = actions; a.M = m; a.q = q; a.acts = acts; a.rstd = rstd;
    hipLaunchKernelGGL(sac_q_fwd_kernel, dim3(ceil_div(m, BM), 2), dim3(256), LDS_BYTES, static_cast<hipStream_t>(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_sac_q_bwd_slabs(int64_t m) { return bwd_slabs(m); }

extern "C" size_t rlx_sac_q_bwd_workspace_bytes(const rlx_sac_q_layout* lay, int64_t m) {
    if (!lay || m <= 0) return 16;
    return (size_t)12 * m * HID * sizeof(float);
}

extern "C" int rlx_sac_q_bwd(const float* params, const rlx_sac_q_layout* lay, const float* states, const float* actions,
                             const float* acts, const float* rstd, const float* d_q, int64_t m, float* grads, int slabs,
                             float* d_actions, void* workspace, size_t workspace_bytes, rlx_stream_t stream) {
    if (int rc = check_q(lay, "rlx_sac_q_bwd")) return rc;
    RLX_REQUIRE(m >= 1, "rlx_sac_q_bwd: empty batch");
    RLX_REQUIRE(grads == nullptr || slabs >= 1, "rlx_sac_q_bwd: slabs=%d", slabs);
    RLX_REQUIRE(params && states && actions && acts && rstd && d_q && workspace, "rlx_sac_q_bwd: NULL argument");
    if (workspace_bytes < rlx_sac_q_bwd_workspace_bytes(lay, m)) {
        set_error("rlx_sac_q_bwd: workspace %zu < %zu bytes", workspace_bytes, rlx_sac_q_bwd_workspace_bytes(lay, m));
        return RLX_ENOSPC;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t MH = (size_t)m * HID;
    float* dz = static_cast<float*>(workspace);
    float* dy = dz + 6 * MH;
    if (int rc = set_lds(sac_q_bwd_dz_kernel)) return rc;
    if (d_actions != nullptr) RLX_HIP_CHECK(hipMemsetAsync(d_actions, 0, (size_t)m * lay->act_dim * sizeof(float), s));
    QBwdArgs b{};
    b.params = params; b.lay = *lay; b.acts = acts; b.rstd = rstd; b.d_q = d_q; b.M = m; b.dz = dz; b.dy = dy;
    b.d_actions = d_actions;
    hipLaunchKernelGGL(sac_q_bwd_dz_kernel, dim3(ceil_div(m, BM), 2), dim3(256), LDS_BYTES, s, b);
    RLX_LAUNCH_CHECK();
    if (grads == nullptr) return RLX_OK;
    const int rows_per_slab = round_up((int)((m + slabs - 1) / slabs), 32);
    DwArgs d{};
    d.M = m; d.n_params = lay->n_params; d.rows_per_slab = rows_per_slab; d.grads = grads;
    ColArgs c{};
    c.M = m; c.n_params = lay->n_params; c.rows_per_slab = rows_per_slab; c.grads = grads;
    for (int y = 0; y < 2; ++y) {
        for (int l = 0; l < 3; ++l) {
            const float* h_prev = l == 0 ? states : acts + (size_t)((y * 3 + l - 1) * 2) * MH;
            d.job[y * 3 + l] = DwJob{dz + (y * 3 + l) * MH, h_prev, l == 0 ? actions : nullptr, l == 0 ? lay->obs_dim : HID,
                                     l == 0 ? lay->act_dim : 0, lay->off_w[y][l], lay->off_b[y][l]};
            const float* hl = acts + (size_t)((y * 3 + l) * 2) * MH;
            c.job[y * 3 + l] = ColJob{dy + (y * 3 + l) * MH, hl + MH, 0, 0, 0, lay->off_g[y][l], lay->off_beta[y][l]};
        }
        c.job[6 + y] = ColJob{d_q, acts + (size_t)((y * 3 + 2) * 2) * MH, lay->out_dim, 2 * lay->out_dim, y * lay->out_dim,
                              lay->off_w[y][3], lay->off_b[y][3]};
    }
    hipLaunchKernelGGL(mlp_dw_kernel, dim3(slabs, 4, 6), dim3(256), 0, s, d);
    RLX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sac_col_kernel, dim3(slabs, 8), dim3(256), 0, s, c);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
