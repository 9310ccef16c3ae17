"""Iteration time of BASELINE config 2 (go2_locomotion, GPU physics + GPU learner, flat terrain) with `policy.activation` -- and the estimator's --
set from the command line: what bench.py measures for the ELU policy, for the reference's other activations.

    python tools/activation_speed.py --activation tanh --num_envs 4096

One process per run; the first failure ends it.  Prints one JSON line.  Timing as bench.py's: 21 untimed iterations (every recording happens there,
the DAgger variants included; the last 5 are the warm-up), then 20 x runner.learn(1) between device synchronisations."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--activation", default="elu", choices=["elu", "selu", "relu", "crelu", "lrelu", "tanh", "sigmoid"])
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="", help="copied into the result line (e.g. which commit ran)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    from quadrupedal_agility_amd.rsl_rl import recording
    torch.cuda.set_device(0)
    cfg = Go2LocomotionCfg()
    cfg.env.num_envs = args.num_envs
    cfg.env.env_id_offset, cfg.env.num_envs_global = 0, args.num_envs
    cfg.terrain.mesh_type = "plane"
    cfg.env.mocap_state_init = False
    cfg.seed = 1
    tcfg = Go2LocomotionCfgAlgo()
    tcfg.runner.amp_enabled = False
    tcfg.policy.activation = args.activation
    tcfg.estimator.activation = args.activation
    cli = get_args(["--device", "gpu", "--device_id", "0"])
    torch.manual_seed(1)
    env, _ = task_registry.make_env("go2_locomotion", args=cli, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=cli, train_cfg=tcfg, log_root=None)
    fallbacks = []
    if hasattr(recording, "capture_failed"):
        inner = recording.capture_failed
        recording.capture_failed = lambda tag, e: (fallbacks.append(tag), inner(tag, e))[1]
    pre = max(0, 21 - args.warmup)
    if pre:
        runner.learn(pre, init_at_random_ep_len=True)
    runner.learn(args.warmup, init_at_random_ep_len=(pre == 0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.learn(1, init_at_random_ep_len=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    alg = runner.alg
    print(json.dumps({"tool": "activation_speed", "tag": args.tag, "activation": args.activation, "num_envs": args.num_envs, "steps": args.steps,
                      "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                      "env_steps_per_s": args.num_envs * runner.num_steps_per_env * args.steps / dt,
                      "update_recorded": bool(getattr(alg, "use_update_graph", False)), "recording_fallbacks": fallbacks,
                      "rollout_chain": bool(runner._policy_chain(False)) if hasattr(runner, "_policy_chain") else None,
                      "train_chain": bool(alg._train_chain_rows(args.num_envs * runner.num_steps_per_env // alg.num_mini_batches))
                      if hasattr(alg, "_train_chain_rows") else None}), flush=True)


if __name__ == "__main__":
    main()
