#!/usr/bin/env python3
"""What the actuator instantiations of the step kernel (qa_set_actuators, include/qa_sim_actuators.h) cost: the env-step time per control type
against the default instantiation on the same box, in interleaved blocks (default, P per joint, V, T, default, ...), by the procedure of
tools/self_collision_hips_cost.py.

    plane     the fused env step alone (200 launches per block, random gaits from reset_all) at 4096 envs, us per launch
    course    the task-level env's physics step (qa_env_physics_step on the generated course, articulated obstacles) at 1024 envs, us per launch
Each twice.  "..._envs": every model with gains and actions of its own kind, free-running -- the scene is the law's (robots under V or T do not
hold a pose), so these rows mix the kernel's cost with the scene's.  "..._envs_same_scene": every model with zero gains and zero actions (zero
torque under every law, the default instantiation included) and every block started from ONE snapshot of the arena: the launches of a block
compute the same physics whatever the model, and the differences are the kernels' alone.
Prints one JSON object and writes it to --out; the numbers go on file as profiles/actuators_cost.json.

  python tools/actuators_cost.py [--blocks 5] [--launches 200] [--skip course] [--out profiles/actuators_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# per-joint P gains around the Go2's 40 / 1; velocity gains of a few N m s / rad, so that the robots of a block keep moving instead of lying folded
MODELS = {"default": None, "P_per_joint": ("P", [30.0, 40.0, 50.0] * 4, [0.8, 1.0, 1.2] * 4), "V": ("V", [4.0, 3.0, 5.0] * 4, [0.01, 0.005, 0.02] * 4),
          "T": ("T", [0.0] * 12, [0.0] * 12)}


def _actuators(model):
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import Actuators
    return None if MODELS[model] is None else Actuators(*MODELS[model])


def _zero(model):
    """the model with zero gains: zero torque under zero actions, whatever the law"""
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import Actuators
    return None if MODELS[model] is None else Actuators(MODELS[model][0], [0.0] * 12, [0.0] * 12)


def plane_job(n, model, same_scene=False):
    import torch
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    h = QaSim(go2_cfg(n, seed=1, **(dict(kp=0.0, kd=0.0, push_robots=0) if same_scene else {})), "cuda:0")
    act = _zero(model) if same_scene else _actuators(model)
    if act is not None:
        h.set_actuators(act)
    h.reset_all()
    g = torch.Generator().manual_seed(2)
    scale = 0.0 if same_scene else 40.0 if model == "T" else 0.5          # action_scale is 0.25: torque actions of a few N m
    acts = [(torch.randn(n, 12, generator=g) * scale).cuda() for _ in range(8)]
    for i in range(50):
        h.step(acts[i % 8])
    torch.cuda.synchronize()
    return h.step, acts, h, None


def course_job(n, model, same_scene=False):
    import torch
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    cfg = Go2AgilityCfg()
    cfg.env.num_envs, cfg.seed, cfg.course_seed = n, 1, 1
    if same_scene:
        cfg.control.stiffness, cfg.control.damping = {"joint": 0.0}, {"joint": 0.0}
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    assert env.actuators is None
    act = _zero(model) if same_scene else _actuators(model)
    if act is not None:
        env.sim.set_actuators(act)                        # behind the constructor: the same course and the same start for every model
    g = torch.Generator().manual_seed(2)
    scale = 0.0 if same_scene else 40.0 if model == "T" else 0.5
    acts = [(torch.randn(n, 12, generator=g) * scale).cuda() for _ in range(8)]
    for i in range(20):
        env.sim.physics_step(acts[i % 8])
    torch.cuda.synchronize()
    return env.sim.physics_step, acts, env.sim, env


def block(job, launches, snapshot=None):
    import torch
    step, acts, sim = job[0], job[1], job[2]
    if snapshot is not None:
        sim.arena.copy_(snapshot); sim.global_step = 50
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        step(acts[i % 8])
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def interleave(jobs, blocks, launches, same_scene=False):
    us = {k: [] for k in jobs}
    snapshot = jobs["default"][2].arena.clone() if same_scene else None      # one start for every block of every model
    for _ in range(blocks):
        for k, job in jobs.items():
            us[k].append(block(job, launches, snapshot))
    out = {"blocks": {k: [round(v, 3) for v in vs] for k, vs in us.items()}, "median": {k: round(statistics.median(vs), 3) for k, vs in us.items()},
           "spread": {k: round(max(vs) - min(vs), 3) for k, vs in us.items()}}
    out["median_difference_to_default"] = {k: round(statistics.median([b - a for a, b in zip(us["default"], vs)]), 3) for k, vs in us.items() if k != "default"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip", nargs="*", default=[], choices=["plane", "course"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    out = {"what": "env-step time of the actuator instantiations (qa_set_actuators) against the default instantiation, interleaved blocks "
                   "(default, P_per_joint, V, T, default, ...), us per launch", "blocks": a.blocks, "launches_per_block": a.launches,
           "device": torch.cuda.get_device_name(0), "models": {k: v for k, v in MODELS.items()}}
    for same in (False, True):
        tag = "_same_scene" if same else ""
        if "plane" not in a.skip:
            jobs = {m: plane_job(4096, m, same) for m in MODELS}
            out["fused_env_step_plane_4096_envs" + tag] = interleave(jobs, a.blocks, a.launches, same)
            del jobs
        if "course" not in a.skip:
            jobs = {m: course_job(1024, m, same) for m in MODELS}
            out["physics_step_course_1024_envs" + tag] = interleave(jobs, a.blocks, a.launches, same)
            del jobs
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
