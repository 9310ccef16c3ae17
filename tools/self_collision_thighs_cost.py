#!/usr/bin/env python3
"""What the calf-against-neighbouring-thigh rows (asset.qa_self_collision_thighs, include/qa_sim_selfcol.h) cost: level 1 (calf-hip rows only)
against level 2 (calf-hip and calf-thigh rows), by the procedure of tools/self_collision_hips_cost.py -- its blocks, its interleaving, its
report ("off" = level 1, "on" = level 2).

    kernel    the fused env step alone (200 launches per block, random gaits from reset_all) at 4096 envs (one workgroup per CU, helper
              wavefronts) and at 16,384 envs (four per CU: 61 KB of LDS rows per workgroup instead of 52), us per launch
    teacher   the task-level teacher at 1024 envs, ms per iteration over blocks of 10 iterations
    bench     one `bench.py --gpus 1 --steps 20 --warmup 5` line with the feature off, in a child process of its own, to set beside the parent
              commit's (the feature's kernels are not on that path)
Prints one JSON object and writes it to --out; the numbers go on file as profiles/self_collision_thighs_cost.json.

  python tools/self_collision_thighs_cost.py [--blocks 5] [--iters 10] [--skip teacher bench] [--out profiles/self_collision_thighs_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import self_collision_hips_cost as hips_cost  # noqa: E402


def kernel_handle(n, thighs):
    h, acts = hips_cost.kernel_handle(n, True)
    if thighs:
        # switched on behind the warm-up steps: the state both handles start their blocks from is the same
        h.set_self_collision_thighs(True)
    return h, acts


def teacher(n, thighs):
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
    cfg.asset.qa_self_collision_hips = True
    cfg.asset.qa_self_collision_thighs = bool(thighs)
    torch.manual_seed(1)
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    runner = OnPolicyRunner(env, class_to_dict(Go2AgilityCfgPPO()), log_dir=None, device="cuda:0")
    runner.learn(21, init_at_random_ep_len=True)          # every recorded variant exists before the clock starts
    runner.learn(3)
    assert env.self_collision_hips and env.self_collision_thighs == bool(thighs)
    return env, runner


def bench_line():
    """the plain benchmark, feature off, in a fresh process"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"bench.py exited with {r.returncode}", "stderr_tail": r.stderr[-400:]}
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip", nargs="*", default=[], choices=["kernel", "teacher", "bench"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"what": "level 1 (asset.qa_self_collision_hips) against level 2 (+ asset.qa_self_collision_thighs), interleaved blocks (1, 2, 1, 2, ...): "
                   "'off' is level 1, 'on' is level 2", "blocks": a.blocks}
    if "kernel" not in a.skip:
        for n in (4096, 16384):
            jobs = {"off": kernel_handle(n, False), "on": kernel_handle(n, True)}
            out[f"env_step_us_per_launch_{n}_envs"] = hips_cost.interleave(jobs, a.blocks, hips_cost.kernel_block)
            del jobs
    if "teacher" not in a.skip:
        jobs = {"off": teacher(1024, False), "on": teacher(1024, True)}
        out["tsc_teacher_1024_envs_ms_per_iteration"] = dict(hips_cost.interleave(jobs, a.blocks, lambda j: hips_cost.learn_block(j, a.iters)), iterations_per_block=a.iters)
        del jobs
    if "bench" not in a.skip:
        import gc
        import torch
        gc.collect(); torch.cuda.empty_cache()
        out["bench_gpus1_steps20_warmup5_feature_off"] = bench_line()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
