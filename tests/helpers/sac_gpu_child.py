"""Child process of tests/test_gpu_sac_policy.py: runs one group of the SAC MLP policy cases on the HIP module on the GPU and
writes the named results (CPU tensors) to a file.  The parent gives it a time limit and compares on the CPU.

    python tests/helpers/sac_gpu_child.py <cases|calls|loop> <out.pt>
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def main(group, out_path):
    from helpers import sac_cases as SC
    from oracle import reference_loader
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    ft = reference_loader.load().mlp_policy.ForwardType
    dev, f32 = torch.device("cuda"), torch.float32
    if group == "cases":
        res = {SC.case_id(*c): SC.run_case(SacMLPPolicy, ft, dev, f32, *c) for c in SC.all_cases()}
    elif group == "calls":
        res = {"stale": SC.run_stale(SacMLPPolicy, ft, dev, f32), "predict": SC.run_predict(SacMLPPolicy, ft, dev, f32)}
    elif group == "loop":
        res = {"loop": SC.run_loop(SacMLPPolicy, ft, dev, f32)}
    else:
        raise SystemExit(f"unknown group {group}")
    torch.cuda.synchronize()
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
