// ppo_loss.hip -- fused PPO clipped-surrogate + clipped-Huber value loss, classic and decoupled (asynchronous), forward and
// backward, gfx950.
//
// Replaces (after rlinf/algorithms/utils.py:280-376 preprocess_loss_inputs):
//   compute_ppo_actor_loss   rlinf/algorithms/losses.py:170-312
//   compute_ppo_critic_loss  rlinf/algorithms/losses.py:315-380  (+ huber_loss utils.py:20-23,
//   masked_mean / masked_mean_ratio rlinf/utils/utils.py:323-356, explained-variance stats
//   rlinf/utils/metric_utils.py:232-258)
// i.e. ~40 elementwise torch kernels + ~15 reductions per micro-batch become ONE streaming pass
// (80 B read per sample at A = 8) + a 1-block finalize; backward is one expand pass (36 B written).
// All scalars (loss, 15 metrics, gradient scales) stay on the device: no .item() syncs.
//
// The per-element derivative is computed in the forward pass, exactly as autograd would for the
// reference graph, including its tie rules: torch.max / torch.min send half the gradient to each
// argument on ties, clamp passes gradient on its closed interval, where() routes to the taken branch.

#include <algorithm>

#include "ppo_loss_math.h"
#include "rlx_common.h"

namespace rlx {
namespace {

using namespace loss;

// One argument block for both losses; prox / versions and the fields of p behind p.ppo are read by the decoupled form only.
struct LossArgs {
    const float *lp, *old, *prox, *versions, *adv, *v, *pv, *ret;
    const uint8_t* m;
    const int64_t* msum;
    float *g_lp, *g_v;
    double* partials;
    long long n;
    rlx_decoupled_loss_params p;
};

// reduction slots: ppo_loss_math.h; the decoupled rows carry one more, the version sum
constexpr int slots(bool decoupled) { return NS + (decoupled ? 1 : 0); }

template <bool DECOUPLED, bool VEC4>
__global__ __launch_bounds__(256) void ppo_loss_fwd_kernel(LossArgs a) {
    constexpr int N = slots(DECOUPLED);
    __shared__ double s_red[N * 4];
    const rlx_ppo_loss_params& p = a.p.ppo;
    const int K = p.raw_per_adv, S = p.sub_per_adv, R = K / S;
    const bool ratio_mode = p.max_episode_steps > 0 && a.m != nullptr && a.msum != nullptr;
    const float half_delta = (float)(0.5 * (double)p.huber_delta);
    const DecoupledMode dm{a.p.proximal_mode, a.p.use_behave_threshold, a.p.behave_weight_threshold, a.p.current_version};
    const bool given = DECOUPLED && dm.mode == RLX_PROX_GIVEN;
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;

    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += stride) {
        const bool on = a.m ? a.m[e] != 0 : true;
        float w = 1.f;
        if (ratio_mode) w = ((float)a.msum[e] * 1.0f) / (float)p.max_episode_steps;
        const float adv = a.adv[e];
        acc[S_NM] += on ? 1.0 : 0.0;
        const float* lpp = a.lp + e * K;
        const float* olp = a.old + e * K;
        const float* pxp = given ? a.prox + e * K : nullptr;
        for (int s = 0; s < S; ++s) {
            float lp = 0.f, old = 0.f, px = 0.f;
            if constexpr (VEC4) {  // the same element order as the scalar loop: the same bits
                for (int j = 0; j < R; j += 4) {
                    if (given) {  // (in front of the other two: 80 VGPRs, the scalar form's occupancy step; behind them 82)
                        const float4 z = *reinterpret_cast<const float4*>(pxp + s * R + j);
                        px = fadd(fadd(fadd(fadd(px, z.x), z.y), z.z), z.w);
                    }
                    const float4 x = *reinterpret_cast<const float4*>(lpp + s * R + j);
                    const float4 y = *reinterpret_cast<const float4*>(olp + s * R + j);
                    lp = fadd(fadd(fadd(fadd(lp, x.x), x.y), x.z), x.w);
                    old = fadd(fadd(fadd(fadd(old, y.x), y.y), y.z), y.w);
                }
            } else {
                for (int j = 0; j < R; ++j) {
                    lp = fadd(lp, lpp[s * R + j]);
                    old = fadd(old, olp[s * R + j]);
                    if (given) px = fadd(px, pxp[s * R + j]);
                }
            }
            float g;
            if constexpr (DECOUPLED) {
                const float vb = a.versions ? a.versions[e * K + s * R] : 0.f;  // the slice's first entry (utils.py:337,348)
                g = decoupled_actor_elem(p, dm, lp, old, px, vb, adv, on, w, ratio_mode, acc, NS);
            } else {
                g = actor_elem(p, lp, old, adv, on, w, ratio_mode, acc);
            }
            a.g_lp[e * S + s] = g;
        }
        if (p.has_critic) a.g_v[e] = critic_elem(p, a.v[e], a.pv[e], a.ret[e], on, w, ratio_mode, half_delta, acc);
    }
    store_partials<N>(acc, s_red, a.partials);
}

template <bool DECOUPLED>
__global__ __launch_bounds__(256) void ppo_loss_finalize(const double* partials, int nparts, long long n_adv,
                                                         rlx_decoupled_loss_params dp, int has_mask, int has_msum, float* out) {
    constexpr int N = slots(DECOUPLED);
    __shared__ double s_red[N * 4];
    double acc[N];
    fold_partials<N>(partials, nparts, acc, s_red);
    if (threadIdx.x != 0) return;
    if constexpr (DECOUPLED) {
        double main[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) main[k] = acc[k];
        finalize_row_decoupled(dp.ppo, dp.use_behave_threshold != 0, n_adv, has_mask != 0, has_msum != 0, main, acc[NS], out);
    } else {
        finalize_row(dp.ppo, n_adv, has_mask != 0, has_msum != 0, acc, out);
    }
}

__global__ __launch_bounds__(256) void ppo_loss_bwd_kernel(const float* g_lp, const float* g_v, const float* out,
                                                           const float* grad_out, float* d_lp, float* d_v,
                                                           long long n_adv, int K, int S) {
    const float go = grad_out ? grad_out[0] : 1.f;
    const float sa = go * out[RLX_PPO_ACTOR_GRAD_SCALE], sc = go * out[RLX_PPO_CRITIC_GRAD_SCALE];
    const int R = K / S;
    const long long total = n_adv * K;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long e = i / K;
        const int s = (int)(i - e * K) / R;
        d_lp[i] = sa * g_lp[e * S + s];
    }
    if (d_v) {
        for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_adv; e += stride) d_v[e] = sc * g_v[e];
    }
}

// The Gaussian policy's entropy does not depend on the state: per row it is sum_a (0.5 + 0.5 log 2pi + logstd_a), so
//   loss -= entropy_bonus * masked_mean(entropy)    (embodied_fsdp_actor_worker.py:679-690, reshape_entropy utils.py:384-408)
// is a constant push on the logstd gradient plus one scalar for the metrics.  elem_scale = 1, or 1/A when entropy_type is
// "token_level" and there is no loss mask (the mean then runs over the [mb, A] elements).
__global__ __launch_bounds__(64) void entropy_bonus_kernel(const float* __restrict__ logstd, int n_act,
                                                           float* __restrict__ grad_logstd, float* __restrict__ out_row,
                                                           float bonus, float grad_scale, int has_mask, float elem_scale,
                                                           const float* __restrict__ actor_scale) {
    const int a = threadIdx.x;
    // behind a decoupled rlx_ppo_step the logstd gradient is in sum form: pre-divide by the scale the slab sum applies later
    const float undo = actor_scale != nullptr ? 1.f / actor_scale[0] : 1.f;
    const float on = (!has_mask || out_row[18] > 0.f) ? 1.f : 0.f;  // masked_mean over an all-False mask is the (zero) sum
    float e = 0.f;
    if (a < n_act) {
        e = 0.5f + 0.91893853320467274178f + logf(expf(logstd[a]));  // Normal.entropy() on scale = exp(logstd)
        grad_logstd[a] -= bonus * grad_scale * elem_scale * on * undo;
    }
    e = wave_sum(e);
    if (a == 0) {
        const float ent_loss = e * elem_scale * on;
        out_row[19] = ent_loss;                                  // actor/entropy_loss
        out_row[RLX_PPO_LOSS] -= bonus * ent_loss;
    }
}

size_t loss_workspace_bytes(bool decoupled) { return (size_t)kPartialBlocks * slots(decoupled) * sizeof(double); }

// What the two forward entry points share: the checks on the common arguments (in `who`'s name) and the two launches.
int loss_fwd(const char* who, bool decoupled, LossArgs& a, float* out, void* workspace, size_t workspace_bytes, rlx_stream_t stream) {
    const rlx_ppo_loss_params* p = &a.p.ppo;
    RLX_REQUIRE(a.n >= 0, "%s: negative size", who);
    RLX_REQUIRE(p->raw_per_adv >= 1 && p->sub_per_adv >= 1 && p->raw_per_adv % p->sub_per_adv == 0,
                "%s: raw_per_adv=%d must be a positive multiple of sub_per_adv=%d", who, p->raw_per_adv, p->sub_per_adv);
    RLX_REQUIRE(a.n == 0 || (a.lp && a.old && a.adv && a.g_lp), "%s: NULL actor argument", who);
    RLX_REQUIRE(!p->has_critic || a.n == 0 || (a.v && a.pv && a.ret && a.g_v), "%s: has_critic set but a critic tensor is NULL", who);
    RLX_REQUIRE(!p->use_dual_clip || p->clip_ratio_c > 1.0f, "clip_ratio_c must be greater than 1.0");  // losses.py:108,262
    RLX_REQUIRE(workspace != nullptr, "%s: NULL workspace", who);
    RLX_REQUIRE_SPACE(workspace_bytes, loss_workspace_bytes(decoupled), who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    a.partials = static_cast<double*>(workspace);
    const int nblk = stream_grid(a.n);
    const int R = p->raw_per_adv / p->sub_per_adv;
    uintptr_t bits = reinterpret_cast<uintptr_t>(a.lp) | reinterpret_cast<uintptr_t>(a.old);
    if (decoupled && a.p.proximal_mode == RLX_PROX_GIVEN) bits |= reinterpret_cast<uintptr_t>(a.prox);
    const bool vec4 = R % 4 == 0 && bits % 16 == 0;
    const int has_mask = a.m != nullptr ? 1 : 0, has_msum = a.msum != nullptr ? 1 : 0;
    if (decoupled) {
        if (vec4) hipLaunchKernelGGL((ppo_loss_fwd_kernel<true, true>), dim3(nblk), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ppo_loss_fwd_kernel<true, false>), dim3(nblk), dim3(256), 0, s, a);
        RLX_LAUNCH_CHECK();
        hipLaunchKernelGGL(ppo_loss_finalize<true>, dim3(1), dim3(256), 0, s, a.partials, nblk, a.n, a.p, has_mask, has_msum, out);
    } else {
        if (vec4) hipLaunchKernelGGL((ppo_loss_fwd_kernel<false, true>), dim3(nblk), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ppo_loss_fwd_kernel<false, false>), dim3(nblk), dim3(256), 0, s, a);
        RLX_LAUNCH_CHECK();
        hipLaunchKernelGGL(ppo_loss_finalize<false>, dim3(1), dim3(256), 0, s, a.partials, nblk, a.n, a.p, has_mask, has_msum, out);
    }
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" size_t rlx_ppo_loss_workspace_bytes(int64_t n_adv) {
    (void)n_adv;
    return loss_workspace_bytes(false);
}

extern "C" size_t rlx_decoupled_loss_workspace_bytes(int64_t n_adv) {
    (void)n_adv;
    return loss_workspace_bytes(true);
}

extern "C" int rlx_ppo_loss_fwd(const float* logprobs, const float* old_logprobs, const float* advantages,
                                const float* values, const float* prev_values, const float* returns,
                                const uint8_t* loss_mask, const int64_t* loss_mask_sum, int64_t n_adv,
                                const rlx_ppo_loss_params* p, float* g_logp, float* g_value, float* out, void* workspace,
                                size_t workspace_bytes, rlx_stream_t stream) {
    RLX_REQUIRE(p != nullptr && out != nullptr, "rlx_ppo_loss_fwd: NULL params/out");
    LossArgs a{};
    a.lp = logprobs, a.old = old_logprobs, a.adv = advantages, a.v = values, a.pv = prev_values, a.ret = returns;
    a.m = loss_mask, a.msum = loss_mask_sum, a.g_lp = g_logp, a.g_v = g_value, a.n = n_adv, a.p.ppo = *p;
    return loss_fwd("rlx_ppo_loss_fwd", false, a, out, workspace, workspace_bytes, stream);
}

// Decoupled (asynchronous) PPO, compute_decoupled_ppo_actor[_critic]_loss rlinf/algorithms/losses.py:27-167,383-393 (inputs:
// rlinf/algorithms/utils.py:310-352; the element math and what "proximal" means: ppo_loss_math.h).  The classic kernels with one
// more reduction slot, and the same backward (rlx_ppo_loss_bwd).
extern "C" int rlx_decoupled_loss_fwd(const float* logprobs, const float* old_logprobs, const float* proximal_logprobs,
                                      const float* versions, const float* advantages, const float* values,
                                      const float* prev_values, const float* returns, const uint8_t* loss_mask,
                                      const int64_t* loss_mask_sum, int64_t n_adv, const rlx_decoupled_loss_params* dp,
                                      float* g_logp, float* g_value, float* out, void* workspace, size_t workspace_bytes,
                                      rlx_stream_t stream) {
    RLX_REQUIRE(dp != nullptr && out != nullptr, "rlx_decoupled_loss_fwd: NULL params/out");
    RLX_REQUIRE(dp->proximal_mode >= RLX_PROX_GIVEN && dp->proximal_mode <= RLX_PROX_FROM_VERSIONS,
                "rlx_decoupled_loss_fwd: unknown proximal_mode %d", dp->proximal_mode);
    RLX_REQUIRE(dp->proximal_mode != RLX_PROX_GIVEN || n_adv == 0 || proximal_logprobs,
                "rlx_decoupled_loss_fwd: proximal_mode GIVEN without proximal_logprobs");
    RLX_REQUIRE(dp->proximal_mode != RLX_PROX_FROM_VERSIONS || n_adv == 0 || versions,
                "rlx_decoupled_loss_fwd: proximal_mode FROM_VERSIONS without versions");
    LossArgs a{};
    a.lp = logprobs, a.old = old_logprobs, a.prox = proximal_logprobs, a.versions = versions, a.adv = advantages;
    a.v = values, a.pv = prev_values, a.ret = returns, a.m = loss_mask, a.msum = loss_mask_sum;
    a.g_lp = g_logp, a.g_v = g_value, a.n = n_adv, a.p = *dp;
    return loss_fwd("rlx_decoupled_loss_fwd", true, a, out, workspace, workspace_bytes, stream);
}

extern "C" int rlx_ppo_loss_bwd(const float* g_logp, const float* g_value, const float* out, const float* grad_out,
                                float* d_logprobs, float* d_values, int64_t n_adv, int raw_per_adv, int sub_per_adv,
                                rlx_stream_t stream) {
    RLX_REQUIRE(n_adv >= 0 && raw_per_adv >= 1 && sub_per_adv >= 1 && raw_per_adv % sub_per_adv == 0,
                "rlx_ppo_loss_bwd: bad sizes");
    if (n_adv == 0) return RLX_OK;
    RLX_REQUIRE(g_logp && out && d_logprobs, "rlx_ppo_loss_bwd: NULL argument");
    RLX_REQUIRE(d_values == nullptr || g_value != nullptr, "rlx_ppo_loss_bwd: d_values requested without g_value");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ppo_loss_bwd_kernel, dim3(stream_grid(n_adv * raw_per_adv)), dim3(256), 0, s, g_logp, g_value, out,
                       grad_out, d_logprobs, d_values, (long long)n_adv, raw_per_adv, sub_per_adv);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

namespace {
int entropy_bonus_launch(const float* logstd, int n_act, float* grad_logstd, float* out_row, float entropy_bonus, float grad_scale,
                         int has_mask, float elem_scale, const float* actor_scale, rlx_stream_t stream) {
    RLX_REQUIRE(logstd && grad_logstd && out_row && n_act >= 1 && n_act <= 64, "rlx_gaussian_entropy_bonus: bad argument");
    hipLaunchKernelGGL(entropy_bonus_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), logstd, n_act,
                       grad_logstd, out_row, entropy_bonus, grad_scale, has_mask, elem_scale, actor_scale);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
}  // namespace

extern "C" int rlx_gaussian_entropy_bonus(const float* logstd, int n_act, float* grad_logstd, float* out_row,
                                          float entropy_bonus, float grad_scale, int has_mask, float elem_scale,
                                          rlx_stream_t stream) {
    return entropy_bonus_launch(logstd, n_act, grad_logstd, out_row, entropy_bonus, grad_scale, has_mask, elem_scale, nullptr, stream);
}

extern "C" int rlx_gaussian_entropy_bonus_deferred(const float* logstd, int n_act, float* grad_logstd, float* out_row,
                                                   float entropy_bonus, float grad_scale, int has_mask, float elem_scale,
                                                   const float* actor_scale, rlx_stream_t stream) {
    RLX_REQUIRE(actor_scale != nullptr, "rlx_gaussian_entropy_bonus_deferred: NULL actor_scale");
    return entropy_bonus_launch(logstd, n_act, grad_logstd, out_row, entropy_bonus, grad_scale, has_mask, elem_scale, actor_scale, stream);
}
