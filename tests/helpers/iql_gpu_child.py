"""Child process of tests/test_gpu_iql.py: runs one group of the offline-IQL cases on the HIP kernels on the GPU and writes the
named results (CPU tensors) to a file.  The parent gives it a time limit and compares on the CPU.

    python tests/helpers/iql_gpu_child.py <kernels|learner> <out.pt>
"""

import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def main(group, out_path):
    from helpers import iql_cases as C

    dev = torch.device("cuda")
    if group == "kernels":
        res = {C.case_id(*c): C.hip_case(*c, dev) for c in C.all_cases()}
        res["optim"] = C.hip_optim(dev, C.ref_optim(torch.float64)[1])
    elif group == "learner":
        res = {f"loop-m{m}": C.hip_loop(m, dev) for m in (32, 67)}
        with tempfile.TemporaryDirectory(prefix="iql_ckpt_") as d:
            res["run_training"] = C.hip_run_training(dev, d)
    else:
        raise SystemExit(f"unknown group {group}")
    torch.cuda.synchronize()
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
