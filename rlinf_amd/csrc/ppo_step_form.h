// ppo_step_form.h -- the precision form of a fused-step call, shared by the step's entry points (ppo_step.hip) and the optimizer's
// weight-image refresh (adamw_clip.hip).
#pragma once

namespace rlx {
namespace step {

// The values are the ones the optimizer kernels read in rlx_adamw_params.tiles_bf16 once the image format is resolved.
enum class Form : int {
    F32 = 0,   // exact-f32 MFMA (ppo_step_f32.hip); the f32 weight image is plain f32 fragment tiles
    BF16 = 1,  // bf16 operands, f32 accumulate (ppo_step_bf16.hip)
    F32X = 2,  // f32 through three bf16 planes on the bf16 matrix pipe (ppo_step_f32x.hip): the default precision-"32" form
};

// The form of a call: bf16 as the caller asks; f32 is F32X unless RLX_F32_EXACT_MFMA=1 (read once per process) selects F32.  The f32
// weight image (rlx_mlp_pack_tiles / the optimizer's tile refresh) follows the same switch.
Form form_of(bool bf16);

}  // namespace step
}  // namespace rlx
