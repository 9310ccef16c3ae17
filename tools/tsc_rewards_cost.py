#!/usr/bin/env python3
"""What the task-level tree's extra reward terms (include/qa_tsc_rewards.h) cost the goal step: us per launch of qa_tsc_goal_step at
1024 and 8192 envs (tests/golden/tsc_env.npz tiled), timed with device events over blocks of back-to-back launches.

    --mode off    qa_tsc_goal_step: the launch of a default run
    --mode on     qa_tsc_goal_step_rewards with all fourteen terms scaled

One measurement per process (--root chooses the checkout whose package and library are measured).  For the parent-against-branch claim
run, in ONE GPU visit,
    parent (--root <parent checkout> --mode off), branch off, parent again, branch on
each with --out, then
    --combine parent1.json off.json parent2.json on.json --out profiles/tsc_rewards_cost.json
which puts the four side by side: the two parent runs give the parent's own run-to-run spread (the range of all their blocks), the median
of "off" must lie within it at every env count (exit status 1 otherwise), "on" is reported as it comes out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

SCALES = (-0.5, -1.0, -1e-3, -2.5e-7, -0.5, -10.0, -5.0, 15.0, -2.0, -1.0, -2.0, -1.0, -0.2, -1e-3)       # tools/gen_golden_tsc_rewards.py


def measure(a, n):
    import numpy as np
    import torch
    from quadrupedal_agility_amd import _capi
    from tests import tsc_env_protocol as proto
    lib = _capi.load_library()
    fx = proto.load_fixture()
    n0 = fx["goal_cur_goal_idx0"].shape[0]
    reps = n // n0
    be = proto.TorchBackend(lib)
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))         # noqa: E731
    tag = "goal_c0_t0_"
    dev = {k: be.put(tile(v)) for k, v in dict(
        root_states=fx[tag + "root_states"], contact_forces=fx[tag + "contact_forces"], rigid_body_states=fx[tag + "rigid_body_states"],
        env_goals=fx["goal_env_goals"], obstacle_types=fx["goal_obstacle_types"].astype(np.int64), action_hl_history=fx[tag + "action_hl_history"],
        episode_length=fx["goal_episode_length0"].astype(np.int64), cur_goal_idx=fx["goal_cur_goal_idx0"].astype(np.int64),
        reach_goal_timer=fx["goal_timer0"], last_contacts=fx["goal_last_contacts0"], cur_goals=fx["goal_cur_goals0"],
        next_goals=fx["goal_next_goals0"]).items()}
    dev["x_edge_mask"] = be.put(fx["goal_x_edge_mask"])
    sums = torch.zeros(8 + 14, n, device="cuda")
    dev["episode_sums"] = sums[:8]
    for k, (w, dt) in proto.OUT_SHAPES.items():
        dev[k] = be.put(np.zeros((n, w) if w else (n,), dt))
    cfg = proto.goal_cfg(fx, n, 0)
    io = _capi.QaTscGoalIo()
    for name in _capi.TSC_GOAL_IO_FIELDS:
        setattr(io, name, dev[name].data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if a.mode == "on":
        g = torch.Generator().manual_seed(1)
        x = _capi.QaTscExtraRewards()
        for i, s in enumerate(SCALES):
            x.scale_dt[i] = s * 0.02
        x.inv_dt = 50.0
        for i in range(12):
            x.default_dof_pos[i], x.dof_pos_lower[i], x.dof_pos_upper[i], x.dof_vel_limit_soft[i], x.torque_limit_soft[i] = 0.5, -1.0, 1.0, 20.0, 8.0
        keep = {k: (torch.randn(n, 24 if k == "dof_state" else 12, generator=g) * 3).cuda() for k in _capi.TSC_EXTRA_POINTERS[:6]}
        for k, t in keep.items():
            setattr(x, k, t.data_ptr())
        x.extra_episode_sums = sums[8:].data_ptr()
        call = lambda: lib.qa_tsc_goal_step_rewards(C.byref(cfg), C.byref(io), C.byref(x), st)      # noqa: E731
    else:
        call = lambda: lib.qa_tsc_goal_step(C.byref(cfg), C.byref(io), st)                           # noqa: E731
    for _ in range(200):
        assert call() == 0
    torch.cuda.synchronize()
    us = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    return {"us_per_launch": [round(v, 3) for v in us], "median_us_per_launch": round(statistics.median(us), 3), "spread_us_per_launch": round(max(us) - min(us), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mode", choices=("off", "on"), default="off")
    ap.add_argument("--num_envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=2000, help="launches per timed block")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs=4, metavar=("PARENT1", "OFF", "PARENT2", "ON"), default=None)
    a = ap.parse_args()
    if a.combine:
        return combine(a)
    sys.path.insert(0, os.path.abspath(a.root))
    out = {"label": a.label, "mode": a.mode, "launches_per_block": a.launches, "note": "launch-to-launch time of back-to-back launches from the host",
           "envs": {str(n): measure(a, n) for n in a.num_envs}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def combine(a):
    p1, off, p2, on = (json.loads(open(f).read()) for f in a.combine)
    assert p1["mode"] == p2["mode"] == off["mode"] == "off" and on["mode"] == "on" and p1["label"] == p2["label"] != off["label"]
    out = {"order": ["parent_1", "branch_off", "parent_2", "branch_on"], "parent_1": p1, "branch_off": off, "parent_2": p2, "branch_on": on, "summary": {}}
    ok = True
    for n in off["envs"]:
        blocks = p1["envs"][n]["us_per_launch"] + p2["envs"][n]["us_per_launch"]
        lo, hi, m = min(blocks), max(blocks), off["envs"][n]["median_us_per_launch"]
        inside = bool(lo <= m <= hi)
        ok &= inside
        out["summary"][n] = {"parent_range_us_per_launch": [lo, hi], "off_median_us_per_launch": m, "off_within_parent_range": inside,
                             "on_median_us_per_launch": on["envs"][n]["median_us_per_launch"],
                             "on_cost_us_per_launch": round(on["envs"][n]["median_us_per_launch"] - m, 3)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
