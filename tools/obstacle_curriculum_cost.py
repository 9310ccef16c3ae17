#!/usr/bin/env python3
"""What the armed-but-untriggered obstacle curriculum costs the task-level teacher (BASELINE configs[3] on one GPU: 1024 envs, the
reference's command line), as ms per learn_RL iteration (24 env steps, rollout as one hipGraph replay + the PPO update).

Two jobs in one process on the same course (`obstacle.curriculum = True`, so both train on the easy bars and tyres):
    unarmed   the flag cleared after construction: no curriculum launch, the launch sequence of a default run
    armed     success_rate 0, below the threshold: one qa_tsc_obstacle_curriculum launch per env step that returns after its uniform read
timed in interleaved blocks (U A U A ...).  The armed cost per env step is (armed - unarmed) / 24.

For the parent-against-branch claim (unarmed == parent within the parent's own run-to-run spread) run `--unarmed-only --curriculum-off`
from a checkout of the parent and of the branch alternately in one GPU visit (P B P B P, `--label parent` / `--label branch`) and put the
JSON lines side by side.  Prints one JSON object and writes it to --out when given; numbers go on file as profiles/obstacle_curriculum_cost.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(n, curriculum, armed):
    import torch
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import class_to_dict
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg, Go2AgilityCfgPPO
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    cfg = Go2AgilityCfg()
    cfg.env.num_envs, cfg.seed, cfg.course_seed = n, 1, 1
    d = cfg.domain_rand
    d.randomize_base_mass = d.randomize_base_com = d.push_robots = True
    cfg.obstacle.randomize_start = True
    cfg.obstacle.curriculum = bool(curriculum)
    torch.manual_seed(1)
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    if not armed:
        env.cfg.obstacle.curriculum = False
    runner = OnPolicyRunner(env, class_to_dict(Go2AgilityCfgPPO()), log_dir=None, device="cuda:0")
    runner.learn(21, init_at_random_ep_len=True)          # both rollout variants recorded (the DAgger one at iteration 20), untimed
    runner.learn(3)
    return env, runner


def block(runner, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runner.learn(iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="iterations per timed block; every 20th iteration is the DAgger variant, so both jobs run the same count")
    ap.add_argument("--unarmed-only", action="store_true")
    ap.add_argument("--curriculum-off", action="store_true", help="build the default course (obstacle.curriculum False): the configuration of a default bench run")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    jobs = {"unarmed": make(a.num_envs, not a.curriculum_off, False)}
    if not a.unarmed_only:
        jobs["armed"] = make(a.num_envs, True, True)
        assert jobs["armed"][0].obstacle_curriculum_armed and not jobs["unarmed"][0].obstacle_curriculum_armed
    ms = {k: [] for k in jobs}
    for _ in range(a.blocks):
        for k, (_env, runner) in jobs.items():
            ms[k].append(block(runner, a.iters))
    out = {"label": a.label, "num_envs": a.num_envs, "iterations_per_block": a.iters, "env_steps_per_iteration": 24,
           "ms_per_iteration": {k: [round(v, 3) for v in vs] for k, vs in ms.items()},
           "median_ms_per_iteration": {k: round(statistics.median(vs), 3) for k, vs in ms.items()},
           "spread_ms_per_iteration": {k: round(max(vs) - min(vs), 3) for k, vs in ms.items()}}
    if "armed" in ms:
        out["armed_cost_us_per_env_step"] = round((statistics.median(ms["armed"]) - statistics.median(ms["unarmed"])) * 1e3 / 24, 2)
        out["armed_raises"] = jobs["armed"][0].obst_curr_count
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
