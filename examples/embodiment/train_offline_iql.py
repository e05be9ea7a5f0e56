#!/usr/bin/env python
"""Offline IQL for the MLP policy on one MI355X (the reference's examples/embodiment/train_offline.py with a d4rl_iql_*.yaml, the
learner's part of it): validate the config, build the learner, call ``run_training`` until ``runner.max_steps``.

    python examples/embodiment/train_offline_iql.py --config-name d4rl_iql_mlp [runner.max_steps=2000 data.dataset_type=npz \
        data.dataset_path=/data/halfcheetah-medium-v2.npz ...]

``data.dataset_type: npz`` reads a file with D4RL's key names (observations, actions, rewards, terminals, next_observations);
``synthetic`` is a seeded random transition set for a smoke run.  Evaluation roll-outs are not part of this script.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(cfg) -> None:
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.workers.actor.fsdp_iql_policy_worker import EmbodiedIQLFSDPPolicy

    cfg = validate_cfg(cfg)
    learner = EmbodiedIQLFSDPPolicy(cfg)
    learner.init_worker()
    resume = cfg.runner.get("resume_dir", None)
    if resume:
        learner.load_checkpoint(resume)
    max_steps, save_interval = int(cfg.runner.max_steps), int(cfg.runner.get("save_interval", -1))
    save_dir = cfg.runner.get("save_dir", None) or os.path.join(cfg.runner.logger.log_path, cfg.runner.logger.experiment_name)
    step, last_saved = learner._global_step, learner._global_step
    while step < max_steps:
        metrics = learner.run_training()
        step = metrics.pop("__global_step")
        print(json.dumps({"step": step, **{k: round(v, 6) for k, v in metrics.items()}}), flush=True)
        if save_interval > 0 and step - last_saved >= save_interval:
            learner.save_checkpoint(os.path.join(save_dir, f"global_step_{step}"), step)
            last_saved = step


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config-path", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "config"))
    ap.add_argument("--config-name", default="d4rl_iql_mlp")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args()
    from rlinf_amd.config import load_config
    main(load_config(os.path.join(args.config_path, args.config_name + ".yaml"), overrides=args.overrides,
                     search_paths=[args.config_path]))
