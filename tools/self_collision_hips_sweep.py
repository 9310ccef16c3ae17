#!/usr/bin/env python3
"""Which ordered (calf leg, hip leg) relations can come within the contact offset under the URDF joint limits?  

float64, CPU only: a dense grid over the calf leg's three joints and the hip leg's joint 0 (the only joint that moves its hip cylinder),
then a shrinking random search around the grid's best pose.  Shapes: tests/selfcol_hips_ref.py (the hip capsule of
tools/self_collision_proximity.py::capsules, the kernel's calf capsule).  A relation whose smallest gap stays above the 0.01 m contact
offset gets no row in csrc/qa_physics.h.

  python tools/self_collision_hips_sweep.py [--out profiles/self_collision_hips_sweep.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.selfcol_hips_ref import CONTACT_OFFSET, DOF_LOWER, DOF_UPPER, LEGS, calf_hip_gap  # noqa: E402


def kind(a, b):
    if a ^ b == 1:
        return "left / right"
    if a ^ b == 2:
        return "front / rear"
    return "diagonal"


def sweep(a, b, rng, grid=(21, 81, 41, 21)):
    lo = np.array([*DOF_LOWER[a], DOF_LOWER[b][0]]); hi = np.array([*DOF_UPPER[a], DOF_UPPER[b][0]])
    axes = [np.linspace(lo[i], hi[i], grid[i]) for i in range(4)]
    best, arg = np.inf, None
    for q0 in axes[0]:                                             # one slab at a time keeps the working set small
        g = np.stack(np.meshgrid([q0], axes[1], axes[2], axes[3], indexing="ij"), -1).reshape(-1, 4)
        gap = calf_hip_gap(g[:, :3], a, np.stack([g[:, 3], 0 * g[:, 3], 0 * g[:, 3]], -1), b)[0]
        i = int(np.argmin(gap))
        if gap[i] < best:
            best, arg = float(gap[i]), g[i].copy()
    width = (hi - lo) / (np.array(grid) - 1)
    for _ in range(30):
        c = np.clip(arg + rng.uniform(-1, 1, (4000, 4)) * width, lo, hi)
        gap = calf_hip_gap(c[:, :3], a, np.stack([c[:, 3], 0 * c[:, 3], 0 * c[:, 3]], -1), b)[0]
        i = int(np.argmin(gap))
        if gap[i] < best:
            best, arg = float(gap[i]), c[i].copy()
        width = width * 0.8
    return best, arg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    for ca in range(4):
        for hb in range(4):
            if ca == hb:
                continue
            g, q = sweep(ca, hb, rng)
            rows.append({"calf_leg": LEGS[ca], "hip_leg": LEGS[hb], "relation": kind(ca, hb), "min_gap_m": round(g, 5),
                         "can_touch": bool(g < CONTACT_OFFSET), "calf_leg_joints_rad": [round(float(v), 4) for v in q[:3]],
                         "hip_leg_joint0_rad": round(float(q[3]), 4)})
            print(rows[-1], flush=True)
    res = {"what": "smallest gap between the calf capsule of one leg and the hip capsule of another over the URDF joint limits (float64 grid "
                   "21 x 81 x 41 x 21 over calf-leg joints 0-2 and hip-leg joint 0, then a shrinking random search); a relation gets a "
                   "contact row in the env step when it can come within the contact offset",
           "contact_offset_m": CONTACT_OFFSET, "relations": rows}
    txt = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
