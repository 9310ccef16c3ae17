#!/usr/bin/env python3
"""What the course mode of the frame renderer costs (include/qa_render_course.h): microseconds per qa_render_frames launch at 640 x 360 on
a generated 4-env course, K = 1 and K = 16 cameras (the four envs, repeated), with the flag off (qa_render_kernel, the static maps) and on
(qa_render_course_kernel: obstacles in their joint state and goals).  Device events around blocks of launches, the blocks of the two modes
interleaved (off, on, off, ...), the median over the blocks and their spread.  The renderer is off the training path: there is no target.

  python tools/render_course_cost.py [--blocks 7] [--launches 50] [--out profiles/render_course_cost.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_course_cost.json"))
    args = ap.parse_args()
    import torch
    from quadrupedal_agility_amd.render import COURSE_OFFSET, FrameRecorder
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    from tools.render_cost import measure
    out = dict(size="640x360", blocks=args.blocks, launches_per_block=args.launches, unit="us per launch (device events)", cases={})
    course = lr.LeggedRobot(make_cfg(4, 3), sim_device="cuda:0")
    act = torch.zeros(4, 12, device="cuda:0")
    for _ in range(5):
        course.step(act)
    for k in (1, 16):
        kw = dict(env_ids=tuple(i % 4 for i in range(k)), size=(640, 360), offset=COURSE_OFFSET)
        off, on = FrameRecorder(course, "unused", **kw), FrameRecorder(course, "unused", articulated=True, goals=True, **kw)
        out["cases"][f"course_K{k}"] = measure({"flag_off": off.render, "flag_on": on.render}, args.blocks, args.launches)
    out["course_map"] = list(course.sim.t["HEIGHT_SAMPLES"].shape)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
