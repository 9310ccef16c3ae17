#!/usr/bin/env python3
"""What measuring the articulated obstacles (obstacle.qa_scan_articulated, include/qa_tsc_scan_obstacles.h) costs the observation launch: the
teacher at 1024 envs on a generated course, flag off (qa_tsc_observations) against flag on (qa_tsc_observations_obstacles on the course's
descriptors, see-saws between their stops, bars and tyres within +-0.05 m), by the procedure of tools/depth_obstacles_cost.py: interleaved
blocks (off, on, off, on, ...), device events around a block of launches, medians, block spread and per-pair differences.  "off" IS the
static observation launch of the same run: the figure to set the difference beside.  Two placements: robots near goals of their course
(tests/test_tsc_depth.py course_scene), where most wavefronts of the overlay leave early, and every robot on a plank or 0.2 .. 1.0 m in
front of a bar or tyre (tests/scan_obstacles_scenes.py), the costly case.

  python tools/scan_obstacles_cost.py [--envs 1024] [--blocks 7] [--launches 200] [--out profiles/scan_obstacles_cost.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scene(n, on_obstacles):
    """root (n,13), map, desc (n,3,8), state (n,3,4) as numpy arrays"""
    import numpy as np
    from tests import depth_obstacles_scenes as dsc
    from tests import scan_obstacles_scenes as sc
    if on_obstacles:
        p = sc.placed(tuple((sc.SEESAW, sc.BAR, sc.TYRE)[i % 3] for i in range(n)), 2, n)
        return p["root"], p["hmap"], p["desc"], p["state"]
    from tests.test_tsc_depth import course_scene
    ob, root, _, _ = course_scene(n, 1)
    rng = np.random.default_rng(1)
    state = np.zeros((n, 3, 4), np.float32)
    state[:, 0, 0] = rng.uniform(-dsc.MAX_TILT, dsc.MAX_TILT, n); state[:, 1:, 0] = rng.uniform(-0.05, 0.05, (n, 2))
    return root.numpy(), np.ascontiguousarray(ob.height_field_raw), dsc.course_descriptors(ob, n), state


def make_jobs(n, on_obstacles):
    import torch
    from quadrupedal_agility_amd import _capi
    from quadrupedal_agility_amd.tsc.legged_gym.task_level import QaTscScanObstacles
    from tests import scan_obstacles_scenes as sc
    root, hmap, desc, state = scene(n, on_obstacles)
    t = {k: v.cuda() for k, v in sc.obs_tensors(n, root, hmap).items()}
    desc, state = torch.from_numpy(desc).cuda(), torch.from_numpy(state).cuda()
    cfg, io = sc.obs_cfg(n, *hmap.shape), sc.obs_io(t)
    obst = QaTscScanObstacles(desc.data_ptr(), state.data_ptr())
    lib = _capi.load_library()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"observation launch failed with code {rc}: {lib.qa_last_error()}")
    jobs = {"off": lambda: check(lib.qa_tsc_observations(C.byref(cfg), C.byref(io), st)),
            "on": lambda: check(lib.qa_tsc_observations_obstacles(C.byref(cfg), C.byref(io), C.byref(obst), st))}
    # what the overlay rewrites: the share of the envs with a covered point, of the scan entries
    jobs["off"](); torch.cuda.synchronize()
    before = t["measured_heights"].clone()
    jobs["on"](); torch.cuda.synchronize()
    moved = t["measured_heights"] != before
    share = {"envs_with_a_rewritten_height": round(moved.any(1).float().mean().item(), 4), "rewritten_heights": round(moved.float().mean().item(), 4)}
    return jobs, (t, desc, state, cfg, io, obst), share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from depth_obstacles_cost import interleave
    if not torch.cuda.is_available():
        raise SystemExit("scan_obstacles_cost.py measures on the GPU: none found")
    out = {"what": "the observation launch, obstacle.qa_scan_articulated off (qa_tsc_observations) against on (qa_tsc_observations_obstacles: the same "
                   "launch and the overlay behind it), us per call, interleaved blocks (off, on, ...)",
           "envs": a.envs, "blocks": a.blocks, "launches_per_block": a.launches}
    for name, on_obstacles in (("robots_near_goals", False), ("robots_on_planks_and_in_front_of_bars_and_tyres", True)):
        jobs, keep, share = make_jobs(a.envs, on_obstacles)
        out[name] = dict(share, **interleave(jobs, a.blocks, a.launches))
        del jobs, keep
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
