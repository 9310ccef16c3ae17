#!/usr/bin/env python3
"""What recovery-pose resets and the contact-set masks (include/qa_sim_reset.h) cost the fused env step: us per step of the 4096-env plane
handle (BASELINE config 2's env count, training exports), timed with device events over blocks of consecutive steps.  The protocol of
tools/extra_rewards_cost.py.

    --mode off    neither setter called: the launch of a default run (the masks and the probability still travel in its arguments)
    --mode on     qa_set_recovery_init(--prob, default 0.2)

One measurement per process (the library is chosen at import: QA_LIB, or --root for a checkout of another commit, whose package
and library are then the ones measured).  For the parent-against-branch claim run, in ONE GPU visit,
    parent (--root <parent checkout> --mode off), branch off, parent again, branch on
each with --out, then
    --combine parent1.json off.json parent2.json on.json --out profiles/recovery_init_cost.json
which puts the four side by side: the two parent runs give the parent's own run-to-run spread (the range of all their blocks), the median
of "off" must lie within it (exit status 1 otherwise), "on" is reported.  Every run also hashes ROOT_STATES, DOF_STATE, OBS, REW and
EPISODE_SUMS after its 100 warm-up steps: parent and "off" must agree (the default path computes what it computed), "on" must not.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mode", choices=("off", "on"), default="off")
    ap.add_argument("--prob", type=float, default=0.2)
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--lean", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300, help="env steps per timed block")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs=4, metavar=("PARENT1", "OFF", "PARENT2", "ON"), default=None)
    a = ap.parse_args()
    if a.combine:
        return combine(a)
    sys.path.insert(0, a.root)
    import torch
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    n = a.num_envs
    h = QaSim(go2_cfg(n, seed=1))
    if a.mode == "on":
        h.set_recovery_init(a.prob)
    h.set_lean_exports(a.lean)
    h.reset_all()
    act = (torch.randn(n, 12, generator=torch.Generator().manual_seed(1)) * 0.5).cuda()
    resets = 0
    for _ in range(100):
        h.step(act)
        resets += int((h.t["RESET"] != 0).sum())
    torch.cuda.synchronize()
    sha = hashlib.sha256()
    for name in ("ROOT_STATES", "DOF_STATE", "OBS", "REW", "EPISODE_SUMS"):
        sha.update(h.t[name].cpu().numpy().tobytes())
    us = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            h.step(act)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.steps)
    out = {"label": a.label, "mode": a.mode, "prob": a.prob if a.mode == "on" else 0.0, "num_envs": n, "lean_exports": a.lean, "steps_per_block": a.steps,
           "us_per_env_step": [round(v, 3) for v in us], "median_us_per_env_step": round(statistics.median(us), 3),
           "spread_us_per_env_step": round(max(us) - min(us), 3), "resets_in_warm_up": resets, "state_sha256_after_warm_up": sha.hexdigest()}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def combine(a):
    p1, off, p2, on = (json.loads(open(f).read()) for f in a.combine)
    assert p1["mode"] == p2["mode"] == off["mode"] == "off" and on["mode"] == "on" and p1["label"] == p2["label"] != off["label"]
    blocks = p1["us_per_env_step"] + p2["us_per_env_step"]
    lo, hi = min(blocks), max(blocks)
    m = off["median_us_per_env_step"]
    key = "state_sha256_after_warm_up"
    out = {"order": ["parent_1", "branch_off", "parent_2", "branch_on"], "parent_1": p1, "branch_off": off, "parent_2": p2, "branch_on": on,
           "parent_range_us_per_env_step": [lo, hi], "off_within_parent_range": bool(lo <= m <= hi),
           "off_state_equals_parent_state": bool(p1[key] == p2[key] == off[key]), "on_state_differs": bool(on[key] != off[key]),
           "on_cost_us_per_env_step": round(on["median_us_per_env_step"] - m, 3)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if out["off_within_parent_range"] and out["off_state_equals_parent_state"] else 1


if __name__ == "__main__":
    sys.exit(main())
