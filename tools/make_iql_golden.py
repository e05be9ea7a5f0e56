"""Record tests/golden/iql_step.pt from the REAL reference on the CPU in float64 (needs the reference tree): for the loop
configuration of tests/test_gpu_iql.py at M = 32 and M = 67, the eight metrics and lr_actor of each of the 5 update steps and, per
live parameter tensor after step 5, its 2-norm and 8 dot products with seeded Gaussian vectors.  Recorded results only.

    python tools/make_iql_golden.py
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def main():
    from helpers import iql_cases as C
    from helpers import iql_reference as R
    from helpers import iql_torch as T

    if not R.available():
        raise SystemExit("the reference tree with its IQL files is needed to record the golden file")
    live = {name: [k for k, _ in mod.named_parameters()] for name, mod in T.make_learner((17, 6), torch.float64, **T.LOOP).modules().items()}
    out = {}
    for m in (32, 67):
        res, L = R.run_loop(m, torch.float64, C.loop_batches(m), T.cast, T.LOOP)
        params = {}
        for name, mod in L.modules().items():
            sd = mod.state_dict()
            params.update({f"{name}/{k}": C.probe(sd[k], f"{name}/{k}") for k in live[name]})
        out[f"m{m}"] = {"metrics": res["metrics"], "lr_actor": res["lr_actor"], "params": params}
    path = os.path.join(ROOT, "tests", "golden", "iql_step.pt")
    torch.save(out, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
