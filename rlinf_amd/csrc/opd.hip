// opd.hip -- on-policy distillation (OPD): the advantage and the policy loss, forward and backward, gfx950.
//
// Replaces:
//   compute_opd_advantages   rlinf/algorithms/advantages.py:367-407   (registry name "opd")
//   compute_opd_actor_loss   rlinf/algorithms/losses.py:427-505       (registry name "opd"; masked_mean / masked_mean_ratio
//                            rlinf/utils/utils.py:323-356)
// The advantage is teacher - prev in f32, reshaped and trimmed on the time axis: one elementwise pass that reads the time rows
// it keeps where they lie (any row stride), so a [T+1, ...] input is never copied.  The loss is a streaming pass over
// (logprobs, advantages, mask, mask_sum) with f64 per-block partials and a one-block finalize, as in ppo_loss.hip: no float
// atomics, so a repeated launch gives the same bits.  The backward re-reads advantages, mask and mask_sum and scales by the
// divisor the finalize published: nothing per element is kept between the passes.
//
// Element arithmetic follows the reference's torch graph in f32, op by op:
//   v = (-lp) * adv;  masked_mean:        loss = sum(v * m) / sum(m)          (sum(v * m) when no element is selected)
//                     masked_mean_ratio:  loss = mean((v / ratio) * m),  ratio = (mask_sum * 1.0) / max_episode_steps
//   d lp = -(((go / div) * m [/ ratio]) * adv)   with div = sum(m), 1 or numel, as autograd chains it.
// A mask_sum of 0 makes ratio 0: v / 0 is inf (NaN for v = 0) and the loss and gradients come out NaN, as in the reference.

#include <algorithm>

#include "rlx_common.h"

namespace rlx {
namespace {

constexpr int kOpdAcc = 3;  // sum(v*m) or sum((v/ratio)*m), sum(adv*m), sum(m)

template <typename T>
struct Vec4 {
    T v[4];
};
template <>
struct alignas(16) Vec4<float> {
    float v[4];
};
template <>
struct alignas(8) Vec4<__bf16> {
    __bf16 v[4];
};
template <>
struct alignas(8) Vec4<_Float16> {
    _Float16 v[4];
};

// out[t, j] = float(teacher[t * ts, j]) - float(prev[t * ps, j]) for t < rows, j < inner.  VEC: 4 elements per lane (inner,
// both row strides and both bases are multiples of 4 elements).
template <typename TT, typename PT, bool VEC>
__global__ __launch_bounds__(256) void opd_adv_kernel(const TT* __restrict__ teacher, const PT* __restrict__ prev,
                                                      float* __restrict__ out, long long rows, long long inner, long long ts,
                                                      long long ps) {
    constexpr int W = VEC ? 4 : 1;
    const long long per_row = inner / W, total = rows * per_row;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long t = i / per_row, j = (i - t * per_row) * W;
        if constexpr (VEC) {
            const Vec4<TT> a = *reinterpret_cast<const Vec4<TT>*>(teacher + t * ts + j);
            const Vec4<PT> b = *reinterpret_cast<const Vec4<PT>*>(prev + t * ps + j);
            float4 o;
            o.x = fsub((float)a.v[0], (float)b.v[0]);
            o.y = fsub((float)a.v[1], (float)b.v[1]);
            o.z = fsub((float)a.v[2], (float)b.v[2]);
            o.w = fsub((float)a.v[3], (float)b.v[3]);
            *reinterpret_cast<float4*>(out + t * inner + j) = o;
        } else {
            out[t * inner + j] = fsub((float)teacher[t * ts + j], (float)prev[t * ps + j]);
        }
    }
}

struct OpdLossArgs {
    const float* lp;
    const float* adv;
    const uint8_t* m;
    const void* msum;
    unsigned n;         // elements of logprobs (< 2^31, checked on the host)
    unsigned m_div;     // mask index = e / m_div (1: full shape, A: one entry per row of A)
    unsigned s_div;     // mask_sum index = e / s_div
    int msum_i64;       // 1: mask_sum is int64, 0: f32
    float max_steps;    // > 0: masked_mean_ratio with this max_episode_steps
};

__device__ __forceinline__ float opd_ratio(const OpdLossArgs& a, unsigned e) {
    const unsigned k = e / a.s_div;
    const float s = a.msum_i64 ? (float)static_cast<const int64_t*>(a.msum)[k] : static_cast<const float*>(a.msum)[k];
    return s / a.max_steps;  // (loss_mask_sum * 1.0) / max_episode_steps, in f32
}

__device__ __forceinline__ void opd_elem(const OpdLossArgs& a, unsigned e, float lp, float adv, double (&acc)[kOpdAcc]) {
    const float m = a.m[e / a.m_div] ? 1.f : 0.f;
    float v = fmul(-lp, adv);
    if (a.max_steps > 0.f) v = v / opd_ratio(a, e);
    acc[0] += (double)fmul(v, m);
    acc[1] += (double)fmul(adv, m);
    acc[2] += (double)m;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void opd_loss_fwd_kernel(OpdLossArgs a, double* __restrict__ partials) {
    __shared__ double s_red[kOpdAcc * 4];
    double acc[kOpdAcc] = {0.0, 0.0, 0.0};
    const unsigned stride = gridDim.x * blockDim.x;
    if constexpr (VEC4) {
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n / 4; i += stride) {
            const float4 x = *reinterpret_cast<const float4*>(a.lp + 4 * (size_t)i);
            const float4 y = *reinterpret_cast<const float4*>(a.adv + 4 * (size_t)i);
            opd_elem(a, 4 * i + 0, x.x, y.x, acc);
            opd_elem(a, 4 * i + 1, x.y, y.y, acc);
            opd_elem(a, 4 * i + 2, x.z, y.z, acc);
            opd_elem(a, 4 * i + 3, x.w, y.w, acc);
        }
    } else {
        for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += stride) opd_elem(a, e, a.lp[e], a.adv[e], acc);
    }
    store_partials<kOpdAcc>(acc, s_red, partials);
}

__global__ __launch_bounds__(256) void opd_loss_finalize(const double* __restrict__ partials, int nparts, long long n,
                                                         int ratio_mode, float* __restrict__ out) {
    __shared__ double s_red[kOpdAcc * 4];
    double acc[kOpdAcc];
    fold_partials<kOpdAcc>(partials, nparts, acc, s_red);
    if (threadIdx.x != 0) return;
    const double cnt = acc[2];
    // masked_mean over an all-False mask is the masked SUM (utils.py:326-327); masked_mean_ratio is a plain mean
    const double div = ratio_mode ? (double)n : (cnt > 0.0 ? cnt : 1.0);
    const double mdiv = cnt > 0.0 ? cnt : 1.0;
    const float loss = (float)(acc[0] / div);
    out[RLX_OPD_LOSS] = loss;
    out[RLX_OPD_POLICY_LOSS] = loss;
    out[RLX_OPD_REWARD] = (float)(acc[1] / mdiv);
    out[RLX_OPD_REVERSE_KL] = (float)(-acc[1] / mdiv);
    out[RLX_OPD_GRAD_DIV] = (float)div;
    out[RLX_OPD_MASK_COUNT] = (float)cnt;
    for (int k = RLX_OPD_MASK_COUNT + 1; k < RLX_OPD_OUT_FLOATS; ++k) out[k] = 0.f;  // reserved slots: defined bits
}

template <bool VEC4>
__global__ __launch_bounds__(256) void opd_loss_bwd_kernel(OpdLossArgs a, const float* __restrict__ out,
                                                           const float* __restrict__ grad_out, float* __restrict__ d_lp) {
    const float g = (grad_out ? grad_out[0] : 1.f) / out[RLX_OPD_GRAD_DIV];
    const bool ratio_mode = a.max_steps > 0.f;
    auto elem = [&](unsigned e, float adv) {
        float w = fmul(g, a.m[e / a.m_div] ? 1.f : 0.f);
        if (ratio_mode) w = w / opd_ratio(a, e);
        return -fmul(w, adv);
    };
    const unsigned stride = gridDim.x * blockDim.x;
    if constexpr (VEC4) {
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n / 4; i += stride) {
            const float4 y = *reinterpret_cast<const float4*>(a.adv + 4 * (size_t)i);
            float4 d;
            d.x = elem(4 * i + 0, y.x);
            d.y = elem(4 * i + 1, y.y);
            d.z = elem(4 * i + 2, y.z);
            d.w = elem(4 * i + 3, y.w);
            *reinterpret_cast<float4*>(d_lp + 4 * (size_t)i) = d;
        }
    } else {
        for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += stride) d_lp[e] = elem(e, a.adv[e]);
    }
}

template <typename TT, typename PT>
void launch_adv(const void* teacher, const void* prev, float* out, long long rows, long long inner, long long ts, long long ps,
                hipStream_t s) {
    const bool vec = inner % 4 == 0 && ts % 4 == 0 && ps % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(teacher) % (4 * sizeof(TT)) == 0 &&
                     reinterpret_cast<uintptr_t>(prev) % (4 * sizeof(PT)) == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const TT* t = static_cast<const TT*>(teacher);
    const PT* p = static_cast<const PT*>(prev);
    if (vec) hipLaunchKernelGGL((opd_adv_kernel<TT, PT, true>), dim3(stream_grid(rows * inner / 4)), dim3(256), 0, s, t, p, out, rows, inner, ts, ps);
    else hipLaunchKernelGGL((opd_adv_kernel<TT, PT, false>), dim3(stream_grid(rows * inner)), dim3(256), 0, s, t, p, out, rows, inner, ts, ps);
}

template <typename TT>
int dispatch_prev(const void* teacher, int prev_dtype, const void* prev, float* out, long long rows, long long inner,
                  long long ts, long long ps, hipStream_t s) {
    switch (prev_dtype) {
        case RLX_DTYPE_F32: launch_adv<TT, float>(teacher, prev, out, rows, inner, ts, ps, s); return RLX_OK;
        case RLX_DTYPE_BF16: launch_adv<TT, __bf16>(teacher, prev, out, rows, inner, ts, ps, s); return RLX_OK;
        case RLX_DTYPE_F16: launch_adv<TT, _Float16>(teacher, prev, out, rows, inner, ts, ps, s); return RLX_OK;
        default: set_error("rlx_opd_advantages: prev_dtype %d is not f32 / bf16 / f16", prev_dtype); return RLX_EINVAL;
    }
}

int check_loss_args(const float* logprobs, const float* advantages, const uint8_t* loss_mask, const void* loss_mask_sum,
                    int64_t n, int mask_div, int msum_div, int msum_i64, int max_episode_steps, const char* who) {
    RLX_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "%s: %lld elements; 0 .. 2^31 - 1 are supported", who, (long long)n);
    RLX_REQUIRE(mask_div >= 1 && msum_div >= 1 && n % mask_div == 0 && n % msum_div == 0,
                "%s: mask_div=%d / msum_div=%d must be positive divisors of n=%lld", who, mask_div, msum_div, (long long)n);
    RLX_REQUIRE(max_episode_steps >= 0, "%s: negative max_episode_steps", who);
    RLX_REQUIRE(n == 0 || (logprobs && advantages && loss_mask), "%s: NULL logprobs / advantages / loss_mask", who);
    RLX_REQUIRE(n == 0 || max_episode_steps == 0 || loss_mask_sum, "%s: max_episode_steps given but loss_mask_sum is NULL", who);
    RLX_REQUIRE(msum_i64 == 0 || msum_i64 == 1, "%s: msum_i64 must be 0 or 1", who);
    return RLX_OK;
}

OpdLossArgs make_args(const float* logprobs, const float* advantages, const uint8_t* loss_mask, const void* loss_mask_sum,
                      int64_t n, int mask_div, int msum_div, int msum_i64, int max_episode_steps) {
    OpdLossArgs a;
    a.lp = logprobs; a.adv = advantages; a.m = loss_mask; a.msum = loss_mask_sum;
    a.n = (unsigned)n; a.m_div = (unsigned)mask_div; a.s_div = (unsigned)msum_div; a.msum_i64 = msum_i64;
    a.max_steps = (float)max_episode_steps;
    return a;
}

bool vec4_ok(const float* x, const float* y, int64_t n) {
    return n % 4 == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
}

}  // namespace
}  // namespace rlx

using namespace rlx;

extern "C" int rlx_opd_advantages(const void* teacher, int teacher_dtype, int64_t teacher_row_stride, const void* prev,
                                  int prev_dtype, int64_t prev_row_stride, int64_t rows, int64_t inner, float* out,
                                  rlx_stream_t stream) {
    RLX_REQUIRE(rows >= 0 && inner >= 0, "rlx_opd_advantages: negative size");
    if (rows == 0 || inner == 0) return RLX_OK;
    RLX_REQUIRE(teacher && prev && out, "rlx_opd_advantages: NULL argument");
    RLX_REQUIRE(teacher_row_stride >= inner && prev_row_stride >= inner,
                "rlx_opd_advantages: row strides (%lld, %lld) must be at least the row length %lld",
                (long long)teacher_row_stride, (long long)prev_row_stride, (long long)inner);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    switch (teacher_dtype) {
        case RLX_DTYPE_F32: rc = dispatch_prev<float>(teacher, prev_dtype, prev, out, rows, inner, teacher_row_stride, prev_row_stride, s); break;
        case RLX_DTYPE_BF16: rc = dispatch_prev<__bf16>(teacher, prev_dtype, prev, out, rows, inner, teacher_row_stride, prev_row_stride, s); break;
        case RLX_DTYPE_F16: rc = dispatch_prev<_Float16>(teacher, prev_dtype, prev, out, rows, inner, teacher_row_stride, prev_row_stride, s); break;
        default: set_error("rlx_opd_advantages: teacher_dtype %d is not f32 / bf16 / f16", teacher_dtype); return RLX_EINVAL;
    }
    if (rc != RLX_OK) return rc;
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" size_t rlx_opd_loss_workspace_bytes(int64_t n) {
    (void)n;
    return (size_t)kPartialBlocks * kOpdAcc * sizeof(double);
}

extern "C" int rlx_opd_loss_fwd(const float* logprobs, const float* advantages, const uint8_t* loss_mask, int mask_div,
                                const void* loss_mask_sum, int msum_div, int msum_i64, int64_t n, int max_episode_steps,
                                float* out, void* workspace, size_t workspace_bytes, rlx_stream_t stream) {
    const int rc = check_loss_args(logprobs, advantages, loss_mask, loss_mask_sum, n, mask_div, msum_div, msum_i64,
                                   max_episode_steps, "rlx_opd_loss_fwd");
    if (rc != RLX_OK) return rc;
    RLX_REQUIRE(out != nullptr && workspace != nullptr, "rlx_opd_loss_fwd: NULL out / workspace");
    RLX_REQUIRE_SPACE(workspace_bytes, rlx_opd_loss_workspace_bytes(n), "rlx_opd_loss_fwd");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const OpdLossArgs a = make_args(logprobs, advantages, loss_mask, loss_mask_sum, n, mask_div, msum_div, msum_i64,
                                    max_episode_steps);
    double* partials = static_cast<double*>(workspace);
    const bool vec = vec4_ok(logprobs, advantages, n);
    const int nblk = stream_grid(vec ? n / 4 : n);
    if (vec) hipLaunchKernelGGL(opd_loss_fwd_kernel<true>, dim3(nblk), dim3(256), 0, s, a, partials);
    else hipLaunchKernelGGL(opd_loss_fwd_kernel<false>, dim3(nblk), dim3(256), 0, s, a, partials);
    RLX_LAUNCH_CHECK();
    hipLaunchKernelGGL(opd_loss_finalize, dim3(1), dim3(256), 0, s, partials, nblk, (long long)n, max_episode_steps > 0 ? 1 : 0,
                       out);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

extern "C" int rlx_opd_loss_bwd(const float* advantages, const uint8_t* loss_mask, int mask_div, const void* loss_mask_sum,
                                int msum_div, int msum_i64, int64_t n, int max_episode_steps, const float* out,
                                const float* grad_out, float* d_logprobs, rlx_stream_t stream) {
    // logprobs themselves are not needed: pass advantages in their place for the shared checks
    const int rc = check_loss_args(advantages, advantages, loss_mask, loss_mask_sum, n, mask_div, msum_div, msum_i64,
                                   max_episode_steps, "rlx_opd_loss_bwd");
    if (rc != RLX_OK) return rc;
    if (n == 0) return RLX_OK;
    RLX_REQUIRE(out && d_logprobs, "rlx_opd_loss_bwd: NULL out / d_logprobs");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const OpdLossArgs a = make_args(nullptr, advantages, loss_mask, loss_mask_sum, n, mask_div, msum_div, msum_i64,
                                    max_episode_steps);
    const bool vec = vec4_ok(advantages, d_logprobs, n);
    if (vec) hipLaunchKernelGGL(opd_loss_bwd_kernel<true>, dim3(stream_grid(n / 4)), dim3(256), 0, s, a, out, grad_out, d_logprobs);
    else hipLaunchKernelGGL(opd_loss_bwd_kernel<false>, dim3(stream_grid(n)), dim3(256), 0, s, a, out, grad_out, d_logprobs);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}
