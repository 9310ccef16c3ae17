#!/usr/bin/env python3
"""What recording frames costs a play loop: microseconds per qa_render_frames launch (include/qa_render.h) at 640 x 360 -- K = 1 and K = 16
cameras on the plane (the 16-env play engine, follow cameras), K = 1 on a generated 4-env course (floor + ceiling maps) -- and, beside each,
the env step of the same engine in the same run.  Device events around blocks of launches, blocks interleaved (render, step, render, ...),
the median over the blocks and their spread; nothing is compared with a parent: the renderer is new and is not on the training path.

  python tools/render_cost.py [--blocks 7] [--launches 100] [--out profiles/render_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, launches):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / launches


def measure(jobs, blocks, launches):
    import torch
    for fn in jobs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in jobs}
    for _ in range(blocks):
        for k, fn in jobs.items():
            rows[k].append(timed(fn, launches))
    return {k: dict(us_median=statistics.median(v), us_min=min(v), us_max=max(v)) for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_cost.json"))
    args = ap.parse_args()
    import types
    import torch
    from quadrupedal_agility_amd.render import FrameRecorder
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    out = dict(size="640x360", blocks=args.blocks, launches_per_block=args.launches, unit="us per launch (device events)", cases={})

    n = 16
    sim = QaSim(go2_cfg(n, seed=1, export_body_state=1), "cuda:0")
    sim.reset_all()
    act = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        sim.step(act)
    env = types.SimpleNamespace(sim=sim)
    for k in (1, 16):
        rec = FrameRecorder(env, "unused", env_ids=tuple(range(k)), size=(640, 360))
        out["cases"][f"plane_K{k}"] = measure({"render": rec.render, "env_step_16_envs": lambda: sim.step(act)}, args.blocks, args.launches)

    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    course = lr.LeggedRobot(make_cfg(4, 3), sim_device="cuda:0")
    act4 = torch.zeros(4, 12, device="cuda:0")
    for _ in range(5):
        course.step(act4)
    rec = FrameRecorder(course, "unused", env_ids=(0,), size=(640, 360))
    out["cases"]["course_K1"] = measure({"render": rec.render, "env_step_task_level_4_envs": lambda: course.step(act4)}, args.blocks, max(args.launches // 4, 10))
    out["course_map"] = list(course.sim.t["HEIGHT_SAMPLES"].shape)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
