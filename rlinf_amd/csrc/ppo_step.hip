// ppo_step.hip -- the C entry points of the two hot launches of the actor-learner loop.  No kernel lives here: every entry point
// validates, builds the argument structs and dispatches on the call's precision form (step::Form, ppo_step_form.h) through one
// table; the kernels and their launchers are in ppo_step_bf16.hip, ppo_step_f32x.hip and ppo_step_f32.hip.
//
//   rlx_mlp_rollout_step   ONE launch per rollout step: obs-preprocess -> actor + value MLPs -> Gaussian sample,
//                          log-prob, value, written straight into the trajectory-buffer rows; value-only jobs
//                          (bootstrap value of the previous step's terminal observations folded into that step's
//                          reward row; the closing value row) ride in the same grid.
//                          replaces MLPPolicy.predict_action_batch (mlp_policy.py:295-320),
//                          MultiStepRolloutWorker.get_bootstrap_values (huggingface_worker.py:612-627) and
//                          EnvWorker.compute_bootstrap_rewards (env_worker.py:718-758).
//   rlx_ppo_step           one optimizer step's forward + loss + backward in TWO launches: (1) fused forward, loss, loss backward
//                          and backward-data chain per row tile and network, (2) weight gradients as split-K slabs, the head
//                          gradients folded in from the per-tile partials of (1), the metric row finalised by the last block.

#include <stdlib.h>

#include <algorithm>

#include "ppo_step_common.h"

namespace rlx {
namespace step {

static bool f32_split() {  // read once per process
    static const bool split = !(getenv("RLX_F32_EXACT_MFMA") != nullptr && atoi(getenv("RLX_F32_EXACT_MFMA")) != 0);
    return split;
}

Form form_of(bool bf16) { return bf16 ? Form::BF16 : f32_split() ? Form::F32X : Form::F32; }

const FormOps& ops_of(Form f) {
    static const FormOps ops[3] = {
        {tiles_bytes_f32, pack_tiles_f32, launch_rollout_f32, launch_step_f32},      // Form::F32
        {tiles_bytes_bf16, pack_tiles_bf16, launch_rollout_bf16, launch_step_bf16},  // Form::BF16
        {tiles_bytes_f32x, pack_tiles_f32x, launch_rollout_f32x, launch_step_f32x},  // Form::F32X
    };
    return ops[(int)f];
}

}  // namespace step
}  // namespace rlx

using namespace rlx;
using namespace rlx::step;

extern "C" int rlx_mlp_rollout_step(const rlx_rollout_step* r, rlx_stream_t stream) {
    RLX_REQUIRE(r != nullptr, "rlx_mlp_rollout_step: NULL argument struct");
    if (int rc = check_layout(r->layout, "rlx_mlp_rollout_step")) return rc;
    RLX_REQUIRE(r->params != nullptr && r->tiles != nullptr, "rlx_mlp_rollout_step: NULL params / tiles");
    RLX_REQUIRE(r->m >= 0 && r->n_value_jobs >= 0 && r->n_value_jobs <= 2, "rlx_mlp_rollout_step: bad sizes");
    RLX_REQUIRE(r->m == 0 || (r->states && r->action && r->logprob && r->value), "rlx_mlp_rollout_step: NULL policy tensor");
    RolloutArgs a{};
    a.params = r->params; a.tiles = r->tiles; a.lay = *r->layout; a.states = r->states; a.eps = r->eps; a.M = r->m;
    a.action = r->action; a.logprob = r->logprob; a.value = r->value; a.states_copy = r->states_copy;
    const int bm = 16;  // rows per workgroup
    a.tiles_policy = ceil_div(r->m, bm);
    int tv[2] = {0, 0};
    for (int k = 0; k < r->n_value_jobs; ++k) {
        const rlx_value_job& j = r->value_jobs[k];
        RLX_REQUIRE(j.m >= 0 && (j.m == 0 || j.states != nullptr), "rlx_mlp_rollout_step: value job %d has no states", k);
        const bool env_store = j.env_rewards != nullptr;
        RLX_REQUIRE(j.rewards == nullptr || ((env_store || j.flags != nullptr) && j.chunk >= 1),
                    "rlx_mlp_rollout_step: value job %d folds rewards without flags", k);
        RLX_REQUIRE(!env_store || (j.rewards && j.env_terminations && j.env_truncations && j.done_row && j.termination_row && j.truncation_row),
                    "rlx_mlp_rollout_step: value job %d stores env rows but a pointer is NULL", k);
        a.vj[k] = ValueJob{j.states, j.m, j.values, j.rewards, j.flags, j.chunk, j.gamma, j.env_rewards, j.env_terminations,
                           j.env_truncations, j.done_row, j.termination_row, j.truncation_row, j.flag_is_truncation};
        tv[k] = ceil_div(j.m, bm);
    }
    a.tiles_vj0 = tv[0]; a.tiles_vj1 = tv[1];
    const int blocks = 2 * a.tiles_policy + tv[0] + tv[1];
    if (blocks == 0) return RLX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return ops_of(form_of(r->bf16 != 0)).launch_rollout(a, blocks, st);
}

extern "C" size_t rlx_mlp_tiles_bytes(const rlx_mlp_layout* lay) {
    (void)lay;
    return std::max({tiles_bytes_f32(), tiles_bytes_bf16(), tiles_bytes_f32x()});  // any of the image formats fits
}

extern "C" size_t rlx_mlp_tiles_bytes_for(const rlx_mlp_layout* lay, int32_t bf16) {
    (void)lay;
    return ops_of(form_of(bf16 != 0)).tiles_bytes();
}

extern "C" int rlx_mlp_pack_tiles(const float* params, const rlx_mlp_layout* lay, float* tiles, rlx_stream_t stream) {
    if (int rc = check_layout(lay, "rlx_mlp_pack_tiles")) return rc;
    RLX_REQUIRE(params && tiles, "rlx_mlp_pack_tiles: NULL argument");
    return ops_of(form_of(false)).pack(params, *lay, tiles, static_cast<hipStream_t>(stream));
}

extern "C" int rlx_mlp_pack_tiles_bf16(const float* params, const rlx_mlp_layout* lay, void* tiles, rlx_stream_t stream) {
    if (int rc = check_layout(lay, "rlx_mlp_pack_tiles_bf16")) return rc;
    RLX_REQUIRE(params && tiles, "rlx_mlp_pack_tiles_bf16: NULL argument");
    return ops_of(Form::BF16).pack(params, *lay, tiles, static_cast<hipStream_t>(stream));
}

extern "C" int rlx_ppo_step_slabs(const rlx_mlp_layout* lay, int64_t m) {
    if (!lay || m <= 0) return 1;
    return plan_step(lay, m, form_of(false)).slabs;
}

extern "C" int rlx_ppo_step_slabs_for(const rlx_mlp_layout* lay, int64_t m, int32_t bf16) {
    if (!lay || m <= 0) return 1;
    return plan_step(lay, m, form_of(bf16 != 0)).slabs;
}

extern "C" size_t rlx_ppo_step_workspace_bytes(const rlx_mlp_layout* lay, int64_t m) {
    if (!lay || m <= 0) return 256;
    return std::max(plan_step(lay, m, form_of(false)).bytes, plan_step(lay, m, Form::BF16).bytes);  // any launch fits
}

extern "C" int rlx_ppo_step(const rlx_ppo_step_args* s, rlx_stream_t stream) {
    RLX_REQUIRE(s != nullptr && s->loss != nullptr, "rlx_ppo_step: NULL argument struct");
    if (int rc = check_layout(s->layout, "rlx_ppo_step")) return rc;
    const rlx_mlp_layout& lay = *s->layout;
    const rlx_ppo_loss_params& p = *s->loss;
    RLX_REQUIRE(s->m >= 1, "rlx_ppo_step: empty micro-batch");
    RLX_REQUIRE(p.raw_per_adv >= 1 && p.sub_per_adv >= 1 && p.raw_per_adv % p.sub_per_adv == 0 && lay.act_dim % p.raw_per_adv == 0,
                "rlx_ppo_step: raw_per_adv=%d / sub_per_adv=%d do not tile act_dim=%d", p.raw_per_adv, p.sub_per_adv, lay.act_dim);
    RLX_REQUIRE(!p.has_critic || lay.act_dim / p.raw_per_adv == lay.val_dim,
                "rlx_ppo_step: %d advantage elements per row but %d value outputs", lay.act_dim / p.raw_per_adv, lay.val_dim);
    RLX_REQUIRE(!p.use_dual_clip || p.clip_ratio_c > 1.0f, "clip_ratio_c must be greater than 1.0");  // losses.py:262
    RLX_REQUIRE(s->params && s->states && s->action && s->old_logprobs && s->advantages && s->grads && s->out && s->workspace,
                "rlx_ppo_step: NULL argument");
    RLX_REQUIRE(!p.has_critic || (s->prev_values && s->returns), "rlx_ppo_step: has_critic set but a critic tensor is NULL");
    const Form form = form_of(s->bf16 != 0);
    const rlx_decoupled_loss_params* dp = s->decoupled;
    if (dp != nullptr) {
        RLX_REQUIRE(dp->proximal_mode >= RLX_PROX_GIVEN && dp->proximal_mode <= RLX_PROX_FROM_VERSIONS,
                    "rlx_ppo_step: unknown proximal_mode %d", dp->proximal_mode);
        RLX_REQUIRE(dp->proximal_mode != RLX_PROX_GIVEN || s->proximal_logprobs, "rlx_ppo_step: proximal_mode GIVEN without proximal_logprobs");
        RLX_REQUIRE(dp->proximal_mode != RLX_PROX_FROM_VERSIONS || s->versions, "rlx_ppo_step: proximal_mode FROM_VERSIONS without versions");
    }
    const StepPlan pl = plan_step(&lay, s->m, form);
    RLX_REQUIRE(s->slabs == pl.slabs, "rlx_ppo_step: grads holds %d slabs, rlx_ppo_step_slabs() says %d", s->slabs, pl.slabs);
    if (s->workspace_bytes < pl.bytes) {
        set_error("rlx_ppo_step: workspace %zu < %zu bytes", s->workspace_bytes, pl.bytes);
        return RLX_ENOSPC;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(s->workspace);
    StepArgs a{};
    a.params = s->params; a.lay = lay; a.states = s->states; a.action = s->action; a.old_logprobs = s->old_logprobs;
    a.advantages = s->advantages; a.prev_values = s->prev_values; a.returns = s->returns; a.loss_mask = s->loss_mask;
    a.loss_mask_sum = s->loss_mask_sum; a.M = s->m; a.p = p; a.grad_out = s->grad_out;
    a.h = reinterpret_cast<float*>(ws + pl.off_h); a.dz = reinterpret_cast<float*>(ws + pl.off_dz);
    a.head_part = reinterpret_cast<float*>(ws + pl.off_head); a.loss_part = reinterpret_cast<double*>(ws + pl.off_loss);
    a.head_stride = pl.head_stride;
    if (dp != nullptr) {
        a.dec.on = 1;
        a.dec.mode = loss::DecoupledMode{dp->proximal_mode, dp->use_behave_threshold, dp->behave_weight_threshold, dp->current_version};
        a.dec.v_theta_dev = s->current_version_dev; a.dec.proximal = s->proximal_logprobs; a.dec.versions = s->versions;
    }
    DwArgs d{};
    d.lay = lay; d.states = s->states; d.h = a.h; d.dz = a.dz; d.head_part = a.head_part; d.loss_part = a.loss_part;
    d.M = s->m; d.rows_per_slab = pl.rows_per_slab; d.slabs = pl.slabs; d.tiles = pl.loss_slots; d.head_parts = pl.head_parts;
    d.head_stride = pl.head_stride;
    d.gemm_items = pl.slabs * 20; d.grads = s->grads; d.p = p; d.has_mask = s->loss_mask != nullptr;
    d.has_msum = s->loss_mask_sum != nullptr; d.out = s->out;
    d.decoupled = dp != nullptr; d.dec_use_threshold = dp != nullptr && dp->use_behave_threshold != 0;
    const int dw_blocks = round_up(d.gemm_items, 8) + pl.slabs * 2 + 1;
    if (s->tiles != nullptr) {
        a.tiles = s->tiles;
    } else {  // no caller-kept image: pack one into the workspace
        void* tiles = ws + pl.off_tiles;
        a.tiles = static_cast<const float*>(tiles);
        if (int rc = ops_of(form).pack(s->params, lay, tiles, st)) return rc;
    }
    return ops_of(form).launch_step(a, d, ws + pl.off_st, pl.tiles, dw_blocks, st);
}
