// iql_mlp.hip -- the networks, loss legs and target update of offline IQL for the MLP policy, gfx950, f32 only.
//
// Replaces IQLMLPPolicy (rlinf/models/embodiment/mlp_policy/iql_mlp_policy.py: _build_mlp :98-117, iql_forward_actor with
// actions :186-210, iql_forward_critic :271-277, iql_forward_value :279-283), autograd's backward through them, and the loss
// expressions and soft update of EmbodiedIQLFSDPPolicy (rlinf/workers/actor/fsdp_iql_policy_worker.py: iql_expectile_loss :35-38,
// forward_value :408-422, forward_actor :424-447, forward_critic :449-470, soft_update_target_model :846-850).
//
// The networks are Linear -> ReLU repeated, then Linear: no LayerNorm, no tanh.  Work decomposition: rlx_mlp_tile.h (one workgroup
// of four waves per 32-row tile and network; blockIdx.y = network, so the twin critic is ONE launch forward and ONE backward).
// Exactness: as sac_mlp.hip -- the MFMA is an exact-f32 fmaf chain summed in 32-deep pieces; what is cheap runs in f64 and rounds
// once: the head outputs, the log-prob epilogue (its terms cancel), the head / log-std gradients (tensors of one or a few
// elements) and the three loss legs (M values each, one workgroup on rlx_reduce.h).

#include "rlx_mlp_tile.h"

namespace rlx {
namespace {

constexpr int MAX_D = 64, MAX_A = 32;
constexpr double LOG_SQRT_2PI = 0.91893853320467274178, LN_2 = 0.69314718055994530942;
// torch.clamp(-1 + 1e-6, 1 - 1e-6) on a float32 tensor: the bounds are rounded to float32 first
constexpr float ATANH_CLAMP = (float)(1.0 - 1e-6);

// ===================================================================================================
// forward
// ===================================================================================================
struct FwdArgs {
    const float* params;
    rlx_iql_mlp_layout lay;
    const float* xa;      // [m_first][in_a]
    const float* xa2;     // [M - m_first][in_a] or nullptr (then m_first == M)
    const float* xb;      // [M][in_b] or nullptr
    long long m_first, M;
    float* out;           // [n_nets][M][out_dim]
    float* acts;          // [n_nets][n_hidden][M][256] or nullptr
    const float* actions; // [M][out_dim] or nullptr: the actor's log-prob epilogue
    float* logprob;       // [M]
};

__device__ __forceinline__ void relu_epilogue(const f32x16 (&acc)[2], const float* __restrict__ bias, float* Xs,
                                              float* __restrict__ save, long long m0, long long M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, khalf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = wave * 64 + t * 32 + lrow;
        const float b = bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = frag_row(r, khalf);
            const float h = fmaxf(acc[t][r] + b, 0.f);
            Xs[row * XS + col] = h;
            if (save != nullptr && m0 + row < M) save[(size_t)(m0 + row) * HID + col] = h;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double atanh_clamped(float a) { return atanh((double)fminf(fmaxf(a, -ATANH_CLAMP), ATANH_CLAMP)); }

__global__ __launch_bounds__(256) void iql_mlp_fwd_kernel(FwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* sOut = Ws + 2 * WBUF;
    const int y = blockIdx.y, tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_iql_mlp_layout& lay = a.lay;
    const int D = lay.in_a, B = lay.in_b, K = D + B, Kp = round_up(K, 8), n_out = lay.out_dim, nh = lay.n_hidden;
    const size_t MH = (size_t)M * HID;
    // the first layer's input: the rows of xa (then xa2), with xb's beside them; zero-padded to Kp columns and past M
    for (int i = tid; i < BM * Kp; i += 256) {
        const int r = i / Kp, c = i % Kp;
        const long long row = m0 + r;
        float v = 0.f;
        if (row < M) {
            if (c < D) v = row < a.m_first ? a.xa[(size_t)row * D + c] : a.xa2[(size_t)(row - a.m_first) * D + c];
            else if (c < K) v = a.xb[(size_t)row * B + (c - D)];
        }
        Xs[r * XS + c] = v;
    }
    f32x16 acc[2];
    for (int l = 0; l < nh; ++l) {
        if (l == 0) tile_gemm(a.params + lay.off_w[y][0], K, K, Kp, (K % 4) == 0 && (lay.off_w[y][0] % 4) == 0, Xs, Ws, acc);
        else tile_gemm(a.params + lay.off_w[y][l], HID, HID, HID, true, Xs, Ws, acc);
        relu_epilogue(acc, a.params + lay.off_b[y][l], Xs, a.acts ? a.acts + (size_t)(y * nh + l) * MH : nullptr, m0, M);
    }
    head_dots(Xs, a.params + lay.off_w[y][nh], a.params + lay.off_b[y][nh], n_out, sOut);
    __syncthreads();
    for (int idx = tid; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        if (m0 + row < M) a.out[((size_t)y * M + m0 + row) * n_out + o] = sOut[row * 32 + o];
    }
    if (a.logprob == nullptr) return;
    // log-prob of the data set's actions under tanh(Normal(mean, exp(clamp(actor_logstd)))): a handful of elements per row, in
    // f64 and rounded once -- the Normal term and the tanh Jacobian are O(1..15) each and cancel
    double* sTerm = reinterpret_cast<double*>(Ws);  // the chunk buffers are idle
    for (int idx = tid; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        if (m0 + row >= M) continue;
        const double ls = (double)fminf(fmaxf(a.params[lay.off_logstd + o], lay.logstd_lo), lay.logstd_hi);
        const double raw = atanh_clamped(a.actions[(size_t)(m0 + row) * n_out + o]);
        const double z = raw - (double)sOut[row * 32 + o];
        // Normal.log_prob: -((x - loc)**2) / (2*var) - log(scale) - log(sqrt(2*pi))
        const double normal = -(z * z) / (2.0 * exp(2.0 * ls)) - ls - LOG_SQRT_2PI;
        const double x = -2.0 * raw;
        const double softplus = fmax(x, 0.0) + log1p(exp(-fabs(x)));
        sTerm[row * 32 + o] = normal - 2.0 * (LN_2 - raw - softplus);
    }
    __syncthreads();
    if (tid < BM && m0 + tid < M) {
        double s = 0.0;
        for (int o = 0; o < n_out; ++o) s += sTerm[tid * 32 + o];
        a.logprob[m0 + tid] = (float)s;
    }
}

// ===================================================================================================
// backward-data: d_out -> the gradient at every hidden layer's Linear output (ReLU mask h > 0: threshold_backward)
// ===================================================================================================
struct BwdArgs {
    const float* params;
    rlx_iql_mlp_layout lay;
    const float* acts;   // [n_nets][n_hidden][M][256]
    const float* d_out;  // [n_nets][M][out_dim]
    long long M;
    float* dz;           // [n_nets][n_hidden][M][256]
};

__global__ __launch_bounds__(256) void iql_mlp_bwd_dz_kernel(BwdArgs a) {
    extern __shared__ __align__(16) float smem[];
    float* Xs = smem;
    float* Ws = smem + BM * XS;
    float* sOut = Ws + 2 * WBUF;
    const int y = blockIdx.y, tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * BM, M = a.M;
    const rlx_iql_mlp_layout& lay = a.lay;
    const int n_out = lay.out_dim, nh = lay.n_hidden;
    const size_t MH = (size_t)M * HID;
    for (int idx = tid; idx < BM * n_out; idx += 256) {
        const int row = idx / n_out, o = idx % n_out;
        sOut[row * 32 + o] = m0 + row < M ? a.d_out[((size_t)y * M + m0 + row) * n_out + o] : 0.f;
    }
    __syncthreads();
    {
        const float* hl = a.acts + (size_t)(y * nh + nh - 1) * MH;
        float* dzl = a.dz + (size_t)(y * nh + nh - 1) * MH;
        head_back(sOut, a.params + lay.off_w[y][nh], n_out, [&](int row, int j, float s) {
            float dzv = 0.f;
            if (m0 + row < M) {
                dzv = hl[(size_t)(m0 + row) * HID + j] > 0.f ? s : 0.f;
                dzl[(size_t)(m0 + row) * HID + j] = dzv;
            }
            Xs[row * XS + j] = dzv;
        });
    }
    __syncthreads();
    f32x16 acc[2];
    for (int l = nh - 2; l >= 0; --l) {
        tile_gemm_t(a.params + lay.off_w[y][l + 1], Xs, Ws, acc);  // dH_l = dZ_{l+1} . W_{l+1}
        const int lane = tid & 63, wave = tid >> 6, lrow = lane & 31, khalf = lane >> 5;
        const float* hl = a.acts + (size_t)(y * nh + l) * MH;
        float* dzl = a.dz + (size_t)(y * nh + l) * MH;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int col = wave * 64 + t * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = frag_row(r, khalf);
                float dzv = 0.f;
                if (m0 + row < M) {
                    dzv = hl[(size_t)(m0 + row) * HID + col] > 0.f ? acc[t][r] : 0.f;
                    dzl[(size_t)(m0 + row) * HID + col] = dzv;
                }
                Xs[row * XS + col] = dzv;
            }
        }
        __syncthreads();
    }
}

// Head gradients of slab s (thread = hidden column j), accumulated in f64 and rounded once: with out_dim == 1 the head bias
// gradient is a ONE-element tensor, and an f32 running sum over the rows would be its whole error.  grid = (slabs, n_nets)
//   dW[o][j] = sum_rows d_out[row][o] * h[row][j], db[o] = sum_rows d_out[row][o]; the actor's reduced d actor_logstd goes into
//   slab 0 and zero into the others, so that every element of every slab is written.
struct HeadGradArgs {
    rlx_iql_mlp_layout lay;
    const float* h_last[2];  // [M][256] per network
    const float* d_out;      // [n_nets][M][out_dim]
    const float* d_logstd;   // [out_dim] or nullptr
    long long M;
    int rows_per_slab;
    float* grads;
};

__global__ __launch_bounds__(256) void iql_head_grad_kernel(HeadGradArgs a) {
    const int s = blockIdx.x, y = blockIdx.y, j = threadIdx.x;
    const rlx_iql_mlp_layout& lay = a.lay;
    const int n_out = lay.out_dim, nh = lay.n_hidden;
    const long long r_begin = (long long)s * a.rows_per_slab, r_end = min(a.M, r_begin + a.rows_per_slab);
    float* slab = a.grads + (size_t)s * lay.n_params;
    const float* H = a.h_last[y];
    const float* dO = a.d_out + (size_t)y * a.M * n_out;
    for (int o0 = 0; o0 < n_out; o0 += 8) {
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int no = min(8, n_out - o0);
        for (long long row = r_begin; row < r_end; ++row) {
            const double h = (double)H[(size_t)row * HID + j];
            const float* d = dO + (size_t)row * n_out + o0;
#pragma unroll
            for (int o = 0; o < 8; ++o)
                if (o < no) acc[o] = fma((double)d[o], h, acc[o]);
        }
        for (int o = 0; o < no; ++o) slab[lay.off_w[y][nh] + (size_t)(o0 + o) * HID + j] = (float)acc[o];
    }
    if (j < n_out) {
        double sb = 0.0;
        for (long long row = r_begin; row < r_end; ++row) sb += (double)dO[(size_t)row * n_out + j];
        slab[lay.off_b[y][nh] + j] = (float)sb;
        if (y == 0 && lay.off_logstd >= 0) slab[lay.off_logstd + j] = (s == 0 && a.d_logstd != nullptr) ? a.d_logstd[j] : 0.f;
    }
}

// ===================================================================================================
// loss legs: M values each, ONE workgroup
// ===================================================================================================
// value: q_t = min(q1_t, q2_t), diff = q_t - v, w = |expectile - 1[diff < 0]|, loss = mean(w diff^2), d_v = -2 w diff / M
__global__ __launch_bounds__(256) void iql_value_loss_kernel(const float* __restrict__ q_target, const float* __restrict__ v,
                                                             long long M, double expectile, float* __restrict__ d_v,
                                                             float* __restrict__ q_min, float* __restrict__ metrics) {
    __shared__ double scratch[8];
    double acc[2] = {0.0, 0.0};
    const double inv_m = 1.0 / (double)M;
    for (long long i = threadIdx.x; i < M; i += 256) {
        const float q = fminf(q_target[i], q_target[M + i]);
        q_min[i] = q;
        const double diff = (double)q - (double)v[i];
        const double w = fabs(expectile - (diff < 0.0 ? 1.0 : 0.0));
        acc[0] += w * diff * diff;
        acc[1] += (double)v[i];
        d_v[i] = (float)(-2.0 * w * diff * inv_m);
    }
    block_sum<2>(acc, scratch);
    if (threadIdx.x == 0) {
        metrics[RLX_IQL_VALUE_LOSS] = (float)(acc[0] * inv_m);
        metrics[RLX_IQL_V] = (float)(acc[1] * inv_m);
    }
}

// actor: adv = q_t - new_v, e = min(exp(adv T), 100), loss = -mean(e lp), d_lp = -e / M; adv mean and adv.std() (Bessel: NaN at
// M == 1, as torch); then through the log-prob: d_mean = d_lp (raw - mean) / var, d logstd_j = sum_rows d_lp ((raw - mean)^2 / var - 1)
// where lo <= actor_logstd_j <= hi (clamp's gradient, inclusive).  q_min == nullptr: d_lp is given and only the second half runs.
struct ActorLossArgs {
    const float* params;
    rlx_iql_mlp_layout lay;
    const float* q_min;
    const float* new_v;
    const float* logprob;
    const float* mean;     // [M][A]
    const float* actions;  // [M][A]
    long long M;
    double temperature;
    float* d_lp;           // [M]: written (q_min given) or read
    float* d_mean;         // [M][A]
    float* d_logstd;       // [A]
    float* metrics;
};

__global__ __launch_bounds__(256) void iql_actor_loss_kernel(ActorLossArgs a) {
    __shared__ double scratch[8];
    __shared__ double sMean;
    __shared__ double sCol[8][32];
    const long long M = a.M;
    const int tid = threadIdx.x, A = a.lay.out_dim;
    if (a.q_min != nullptr) {
        const double inv_m = 1.0 / (double)M;
        double acc[2] = {0.0, 0.0};
        for (long long i = tid; i < M; i += 256) {
            const double adv = (double)a.q_min[i] - (double)a.new_v[i];
            const double e = fmin(exp(adv * a.temperature), 100.0);
            acc[0] += adv;
            acc[1] += e * (double)a.logprob[i];
            a.d_lp[i] = (float)(-e * inv_m);
        }
        block_sum<2>(acc, scratch);
        if (tid == 0) {
            sMean = acc[0] * inv_m;
            a.metrics[RLX_IQL_ACTOR_LOSS] = (float)(-acc[1] * inv_m);
            a.metrics[RLX_IQL_ADV_MEAN] = (float)(acc[0] * inv_m);
        }
        __syncthreads();
        const double mean = sMean;
        double ss[1] = {0.0};
        for (long long i = tid; i < M; i += 256) {
            const double d = (double)a.q_min[i] - (double)a.new_v[i] - mean;
            ss[0] += d * d;
        }
        block_sum<1>(ss, scratch);
        if (tid == 0) a.metrics[RLX_IQL_ADV_STD] = (float)sqrt(ss[0] / (double)(M - 1));  // M == 1: 0 / 0
        __syncthreads();  // this block's d_lp
    }
    const int j = tid & 31, g = tid >> 5;
    double s = 0.0;
    bool pass = false;
    if (j < A) {
        const float p = a.params[a.lay.off_logstd + j];
        pass = p >= a.lay.logstd_lo && p <= a.lay.logstd_hi;
        const double inv_var = exp(-2.0 * (double)fminf(fmaxf(p, a.lay.logstd_lo), a.lay.logstd_hi));
        for (long long i = g; i < M; i += 8) {
            const double dl = (double)a.d_lp[i];
            const double z = atanh_clamped(a.actions[(size_t)i * A + j]) - (double)a.mean[(size_t)i * A + j];
            a.d_mean[(size_t)i * A + j] = (float)(dl * z * inv_var);
            s += dl * (z * z * inv_var - 1.0);
        }
    }
    sCol[g][j] = s;
    __syncthreads();
    if (tid < A) {
        double tot = 0.0;
        for (int k = 0; k < 8; ++k) tot += sCol[k][tid];
        a.d_logstd[tid] = pass ? (float)tot : 0.f;
    }
}

// critic: target = r + gamma mask next_v, loss = mean((q1 - target)^2 + (q2 - target)^2), d_q_i = 2 (q_i - target) / M
__global__ __launch_bounds__(256) void iql_critic_loss_kernel(const float* __restrict__ q, const float* __restrict__ next_v,
                                                              const float* __restrict__ rewards, const float* __restrict__ masks,
                                                              long long M, double gamma, float* __restrict__ d_q,
                                                              float* __restrict__ metrics) {
    __shared__ double scratch[12];
    double acc[3] = {0.0, 0.0, 0.0};
    const double inv_m = 1.0 / (double)M;
    for (long long i = threadIdx.x; i < M; i += 256) {
        const double target = (double)rewards[i] + gamma * (double)masks[i] * (double)next_v[i];
        const double e1 = (double)q[i] - target, e2 = (double)q[M + i] - target;
        acc[0] += e1 * e1 + e2 * e2;
        acc[1] += (double)q[i];
        acc[2] += (double)q[M + i];
        d_q[i] = (float)(2.0 * e1 * inv_m);
        d_q[M + i] = (float)(2.0 * e2 * inv_m);
    }
    block_sum<3>(acc, scratch);
    if (threadIdx.x == 0) {
        metrics[RLX_IQL_CRITIC_LOSS] = (float)(acc[0] * inv_m);
        metrics[RLX_IQL_Q1] = (float)(acc[1] * inv_m);
        metrics[RLX_IQL_Q2] = (float)(acc[2] * inv_m);
    }
}

// t <- t (1 - tau), then t <- t + tau c: _foreach_mul_(t, 1 - tau) rounds the product, _foreach_add_(t, c, alpha = tau) is one
// fused multiply-add on top of it (torch's vectorised add-with-alpha is fmadd); both scalars are rounded to f32 first
__global__ __launch_bounds__(256) void soft_update_kernel(float* __restrict__ t, const float* __restrict__ c, long long n,
                                                          float one_minus_tau, float tau) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        t[i] = fmaf(tau, c[i], fmul(t[i], one_minus_tau));
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_layout(const rlx_iql_mlp_layout* lay, const char* who) {
    RLX_REQUIRE(lay != nullptr, "%s: NULL layout", who);
    RLX_REQUIRE(lay->hidden == HID, "%s: hidden=%d is not supported (the reference's IQL configs are 256 wide)", who, lay->hidden);
    RLX_REQUIRE(lay->n_nets == 1 || lay->n_nets == 2, "%s: n_nets=%d (1 or 2)", who, lay->n_nets);
    RLX_REQUIRE(lay->n_hidden == 2 || lay->n_hidden == 3, "%s: n_hidden=%d (2 or 3)", who, lay->n_hidden);
    RLX_REQUIRE(lay->in_a >= 1 && lay->in_a <= MAX_D, "%s: in_a (obs_dim)=%d out of range [1,%d]", who, lay->in_a, MAX_D);
    RLX_REQUIRE(lay->in_b >= 0 && lay->in_b <= MAX_A, "%s: in_b (action_dim)=%d out of range [0,%d]", who, lay->in_b, MAX_A);
    RLX_REQUIRE(lay->out_dim >= 1 && lay->out_dim <= MAX_A, "%s: out_dim=%d out of range [1,%d]", who, lay->out_dim, MAX_A);
    const int64_t n = lay->n_params;
    const int nh = lay->n_hidden;
    for (int y = 0; y < lay->n_nets; ++y)
        for (int l = 0; l <= nh; ++l) {
            const int64_t rows = l == nh ? lay->out_dim : HID, cols = l == 0 ? lay->in_a + lay->in_b : HID;
            RLX_REQUIRE(in_range(lay->off_w[y][l], rows * cols, n) && in_range(lay->off_b[y][l], rows, n),
                        "%s: offset of net %d layer %d out of range", who, y, l);
            RLX_REQUIRE(l == 0 || lay->off_w[y][l] % 4 == 0, "%s: offsets of the 256-wide weights must be multiples of 4", who);
        }
    RLX_REQUIRE(lay->off_logstd == -1 || (lay->n_nets == 1 && in_range(lay->off_logstd, lay->out_dim, n)),
                "%s: off_logstd out of range (or -1: none)", who);
    return RLX_OK;
}

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_iql_mlp_fwd(const float* params, const rlx_iql_mlp_layout* lay, const float* xa, int64_t m_first, const float* xa2,
                               const float* xb, int64_t m, float* out, float* acts, const float* actions, float* logprob,
                               rlx_stream_t stream) {
    if (int rc = check_layout(lay, "rlx_iql_mlp_fwd")) return rc;
    RLX_REQUIRE(m >= 0, "rlx_iql_mlp_fwd: negative batch m");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(params && xa && out, "rlx_iql_mlp_fwd: NULL argument (params, xa, out)");
    RLX_REQUIRE(aligned16(params), "rlx_iql_mlp_fwd: params is misaligned (the 256-wide weights are read 16 bytes at a time)");
    RLX_REQUIRE((lay->in_b > 0) == (xb != nullptr), "rlx_iql_mlp_fwd: xb goes with in_b > 0");
    RLX_REQUIRE(xa2 != nullptr ? (m_first >= 1 && m_first < m && xb == nullptr) : m_first == m,
                "rlx_iql_mlp_fwd: m_first=%lld (all of m without xa2; inside [1, m) with it, and then no xb)", (long long)m_first);
    RLX_REQUIRE((actions == nullptr) == (logprob == nullptr), "rlx_iql_mlp_fwd: actions and logprob go together");
    RLX_REQUIRE(actions == nullptr || lay->off_logstd >= 0, "rlx_iql_mlp_fwd: the log-prob needs a layout with actor_logstd");
    if (int rc = set_lds(iql_mlp_fwd_kernel)) return rc;
    FwdArgs a{};
    a.params = params; a.lay = *lay; a.xa = xa; a.xa2 = xa2; a.xb = xb; a.m_first = m_first; a.M = m; a.out = out; a.acts = acts;
    a.actions = actions; a.logprob = logprob;
    hipLaunchKernelGGL(iql_mlp_fwd_kernel, dim3(ceil_div(m, BM), lay->n_nets), dim3(256), LDS_BYTES, static_cast<hipStream_t>(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_iql_mlp_bwd_slabs(int64_t m) { return bwd_slabs(m); }

extern "C" size_t rlx_iql_mlp_bwd_workspace_bytes(const rlx_iql_mlp_layout* lay, int64_t m) {
    if (!lay || m <= 0) return 16;
    return (size_t)lay->n_nets * lay->n_hidden * m * HID * sizeof(float);
}

extern "C" int rlx_iql_mlp_bwd(const float* params, const rlx_iql_mlp_layout* lay, const float* xa, const float* xb, const float* acts,
                               const float* d_out, const float* d_logstd, int64_t m, float* grads, int slabs, void* workspace,
                               size_t workspace_bytes, rlx_stream_t stream) {
    if (int rc = check_layout(lay, "rlx_iql_mlp_bwd")) return rc;
    RLX_REQUIRE(m >= 1, "rlx_iql_mlp_bwd: empty batch m");
    RLX_REQUIRE(slabs >= 1, "rlx_iql_mlp_bwd: slabs=%d", slabs);
    RLX_REQUIRE(params && xa && acts && d_out && grads && workspace, "rlx_iql_mlp_bwd: NULL argument");
    RLX_REQUIRE(aligned16(params) && aligned16(acts) && aligned16(workspace) && aligned16(xa),
                "rlx_iql_mlp_bwd: params, xa, acts or workspace is misaligned (they are read 16 bytes at a time)");
    RLX_REQUIRE((lay->in_b > 0) == (xb != nullptr), "rlx_iql_mlp_bwd: xb goes with in_b > 0");
    RLX_REQUIRE(d_logstd == nullptr || lay->off_logstd >= 0, "rlx_iql_mlp_bwd: d_logstd needs a layout with actor_logstd");
    RLX_REQUIRE_SPACE(workspace_bytes, rlx_iql_mlp_bwd_workspace_bytes(lay, m), "rlx_iql_mlp_bwd");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t MH = (size_t)m * HID;
    const int nh = lay->n_hidden, nn = lay->n_nets;
    float* dz = static_cast<float*>(workspace);
    if (int rc = set_lds(iql_mlp_bwd_dz_kernel)) return rc;
    BwdArgs b{};
    b.params = params; b.lay = *lay; b.acts = acts; b.d_out = d_out; b.M = m; b.dz = dz;
    hipLaunchKernelGGL(iql_mlp_bwd_dz_kernel, dim3(ceil_div(m, BM), nn), dim3(256), LDS_BYTES, s, b);
    RLX_LAUNCH_CHECK();
    const int rows_per_slab = round_up((int)((m + slabs - 1) / slabs), 32);
    DwArgs d{};
    d.M = m; d.n_params = lay->n_params; d.rows_per_slab = rows_per_slab; d.grads = grads;
    HeadGradArgs h{};
    h.lay = *lay; h.d_out = d_out; h.d_logstd = d_logstd; h.M = m; h.rows_per_slab = rows_per_slab; h.grads = grads;
    static_assert(2 * 3 <= MAX_DW_JOBS, "two networks of three hidden layers");
    for (int y = 0; y < nn; ++y) {
        for (int l = 0; l < nh; ++l)
            d.job[y * nh + l] = DwJob{dz + (size_t)(y * nh + l) * MH, l == 0 ? xa : acts + (size_t)(y * nh + l - 1) * MH,
                                      l == 0 ? xb : nullptr, l == 0 ? lay->in_a : HID, l == 0 ? lay->in_b : 0, lay->off_w[y][l],
                                      lay->off_b[y][l]};
        h.h_last[y] = acts + (size_t)(y * nh + nh - 1) * MH;
    }
    hipLaunchKernelGGL(mlp_dw_kernel, dim3(slabs, 4, nn * nh), dim3(256), 0, s, d);
    RLX_LAUNCH_CHECK();
    hipLaunchKernelGGL(iql_head_grad_kernel, dim3(slabs, nn), dim3(256), 0, s, h);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_iql_value_loss(const float* q_target, const float* v, int64_t m, double expectile, float* d_v, float* q_min,
                                  float* metrics, rlx_stream_t stream) {
    RLX_REQUIRE(m >= 0, "rlx_iql_value_loss: negative batch m");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(q_target && v && d_v && q_min && metrics, "rlx_iql_value_loss: NULL argument");
    hipLaunchKernelGGL(iql_value_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), q_target, v, (long long)m,
                       expectile, d_v, q_min, metrics);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_iql_actor_loss(const float* params, const rlx_iql_mlp_layout* lay, const float* q_min, const float* new_v,
                                  const float* logprob, const float* mean, const float* actions, int64_t m, double temperature,
                                  float* d_lp, float* d_mean, float* d_logstd, float* metrics, rlx_stream_t stream) {
    if (int rc = check_layout(lay, "rlx_iql_actor_loss")) return rc;
    RLX_REQUIRE(lay->off_logstd >= 0, "rlx_iql_actor_loss: needs a layout with actor_logstd");
    RLX_REQUIRE(m >= 0, "rlx_iql_actor_loss: negative batch m");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(params && mean && actions && d_lp && d_mean && d_logstd, "rlx_iql_actor_loss: NULL argument");
    RLX_REQUIRE(q_min == nullptr || (new_v && logprob && metrics),
                "rlx_iql_actor_loss: NULL argument (new_v, logprob and metrics go with q_min)");
    ActorLossArgs a{};
    a.params = params; a.lay = *lay; a.q_min = q_min; a.new_v = new_v; a.logprob = logprob; a.mean = mean; a.actions = actions;
    a.M = m; a.temperature = temperature; a.d_lp = d_lp; a.d_mean = d_mean; a.d_logstd = d_logstd; a.metrics = metrics;
    hipLaunchKernelGGL(iql_actor_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_iql_critic_loss(const float* q, const float* next_v, const float* rewards, const float* masks, int64_t m,
                                   double gamma, float* d_q, float* metrics, rlx_stream_t stream) {
    RLX_REQUIRE(m >= 0, "rlx_iql_critic_loss: negative batch m");
    if (m == 0) return RLX_OK;
    RLX_REQUIRE(q && next_v && rewards && masks && d_q && metrics, "rlx_iql_critic_loss: NULL argument");
    hipLaunchKernelGGL(iql_critic_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), q, next_v, rewards, masks,
                       (long long)m, gamma, d_q, metrics);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_soft_update(float* target, const float* online, int64_t n, double tau, rlx_stream_t stream) {
    RLX_REQUIRE(n >= 0, "rlx_soft_update: negative n");
    if (n == 0) return RLX_OK;
    RLX_REQUIRE(target && online, "rlx_soft_update: NULL argument");
    RLX_REQUIRE(tau >= 0.0 && tau <= 1.0, "rlx_soft_update: tau=%g outside [0, 1]", tau);
    hipLaunchKernelGGL(soft_update_kernel, dim3(stream_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), target, online,
                       (long long)n, (float)(1.0 - tau), (float)tau);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
