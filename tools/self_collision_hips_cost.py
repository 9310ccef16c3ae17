#!/usr/bin/env python3
"""What the calf-against-neighbouring-hip rows (asset.qa_self_collision_hips, include/qa_sim_selfcol.h) cost, feature off against on.

Three measurements in one process, each interleaved off / on / off / on ... so that drift of the box hits both alike:
    kernel    the fused env step alone (qa_env_step, HIP events around 200 launches per block, random actions from reset_all) at 4096 envs
              (one workgroup per CU, helper wavefronts) and at 16,384 envs (four per CU: where the larger LDS record could cost occupancy),
              us per launch -- the yardstick is the calf-calf class, 82.8 -> 86.5 us per 4096-env launch
    config3   BASELINE config 3 (AMP, mocap resets) at 4096 envs, ms per iteration over blocks of 10 iterations
    teacher   the task-level teacher at 1024 envs, the same
Reports every block, the medians and the per-pair differences (block i on - block i off).  Prints one JSON object and writes it to --out;
the numbers go on file as profiles/self_collision_hips_cost.json.

  python tools/self_collision_hips_cost.py [--blocks 5] [--iters 10] [--skip teacher] [--out profiles/self_collision_hips_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_handle(n, hips):
    import torch
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    h = QaSim(go2_cfg(n, seed=1, self_collision=1), "cuda:0")
    if hips:
        h.set_self_collision_hips(True)
    h.reset_all()
    g = torch.Generator().manual_seed(2)
    acts = [(torch.randn(n, 12, generator=g) * 0.5).cuda() for _ in range(8)]
    for i in range(50):
        h.step(acts[i % 8])
    torch.cuda.synchronize()
    return h, acts


def kernel_block(job, launches=200):
    import torch
    h, acts = job
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        h.step(acts[i % 8])
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def config3(n, hips):
    import torch
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = True; cfg.seed = 1
    cfg.asset.qa_self_collision_hips = bool(hips)
    t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = True; t.seed = 1; t.runner.save_interval = 10 ** 9
    torch.manual_seed(1)
    args = get_args(["--device", "gpu"])
    env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=None)
    runner.learn(21, init_at_random_ep_len=True)          # every recorded variant exists before the clock starts
    runner.learn(3)
    assert env.self_collision_hips == bool(hips)
    return env, runner


def teacher(n, hips):
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
    cfg.asset.qa_self_collision_hips = bool(hips)
    torch.manual_seed(1)
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    runner = OnPolicyRunner(env, class_to_dict(Go2AgilityCfgPPO()), log_dir=None, device="cuda:0")
    runner.learn(21, init_at_random_ep_len=True)
    runner.learn(3)
    assert env.self_collision_hips == bool(hips)
    return env, runner


def learn_block(job, iters):
    import torch
    _env, runner = job
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runner.learn(iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def interleave(jobs, blocks, fn):
    ms = {k: [] for k in jobs}
    for _ in range(blocks):
        for k, job in jobs.items():
            ms[k].append(fn(job))
    diffs = [b - a for a, b in zip(ms["off"], ms["on"])]
    return {"blocks": {k: [round(v, 3) for v in vs] for k, vs in ms.items()}, "median": {k: round(statistics.median(vs), 3) for k, vs in ms.items()},
            "spread": {k: round(max(vs) - min(vs), 3) for k, vs in ms.items()}, "per_pair_difference_on_minus_off": [round(v, 3) for v in diffs],
            "median_difference": round(statistics.median(diffs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip", nargs="*", default=[], choices=["kernel", "config3", "teacher"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"what": "asset.qa_self_collision_hips off against on, interleaved blocks (off, on, off, on, ...)", "blocks": a.blocks}
    if "kernel" not in a.skip:
        for n in (4096, 16384):
            jobs = {"off": kernel_handle(n, False), "on": kernel_handle(n, True)}
            out[f"env_step_us_per_launch_{n}_envs"] = interleave(jobs, a.blocks, kernel_block)
            del jobs
    if "config3" not in a.skip:
        jobs = {"off": config3(4096, False), "on": config3(4096, True)}
        out["config3_4096_envs_ms_per_iteration"] = dict(interleave(jobs, a.blocks, lambda j: learn_block(j, a.iters)), iterations_per_block=a.iters)
        del jobs
    if "teacher" not in a.skip:
        jobs = {"off": teacher(1024, False), "on": teacher(1024, True)}
        out["tsc_teacher_1024_envs_ms_per_iteration"] = dict(interleave(jobs, a.blocks, lambda j: learn_block(j, a.iters)), iterations_per_block=a.iters)
        del jobs
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
