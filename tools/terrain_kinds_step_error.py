#!/usr/bin/env python3
"""Share of env-steps outside tests/parity_tol.py's TOL, HIP against the CPU oracle, on the map with one tile of each terrain kind beyond the
slopes (tests/test_terrain_kinds.py's procedure, `run_parity`): robots reset on the tiles' platforms, and robots dropped with their feet
across a riser, a block edge, a stone's end and the gap's rim.  1, 64, 67 and 600 envs, 10 steps each, per case.

Writes profiles/terrain_kinds_step_error.json with the kernel-source hash; the steep case's share is what STEEP_BUDGET in
tests/test_terrain_kinds.py is twice of (quoted beside the constant there).  Needs a GPU.

  python tools/terrain_kinds_step_error.py [--out profiles/terrain_kinds_step_error.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = ((1, 3), (64, 2), (67, 11), (600, 7))          # (envs, seed): the test's parametrisation and a larger sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_kinds_step_error.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    import bench
    g.build()
    import tests.test_terrain_kinds as K
    out = {"protocol": "tests/test_terrain_kinds.py::run_parity: 10 random-action env steps, each from the oracle's arena, every fourth env saturating; an env-step "
                       "counts when any tensor of tests/parity_tol.py's TOL (or SCAN_HEIGHT, exactly) is outside its tolerance.  steep: env e at site e % 4 "
                       "(riser below the stairs' top, block edge, stone's end, rim of the gap); platforms: env e reset on the platform of tile e % 6",
           "device": "MI355X", "horizon": K.HORIZON, "kernel_source_hash": bench.env_kernel_hash(g), "runs": []}
    for which, place in (("steep", K.place_on_steep_cells), ("platforms", None)):
        f_all = t_all = 0
        for n, seed in RUNS:
            flips, total, per_env, _, _ = K.run_parity(n, seed, place=place)
            out["runs"].append({"case": which, "n_envs": n, "seed": seed, "outside": flips, "env_steps": total, "share": flips / total,
                                "median_error": {k: float(np.median(np.concatenate(v))) for k, v in per_env.items()}})
            f_all += flips; t_all += total
        out[which + "_outside"], out[which + "_env_steps"], out[which + "_share"] = f_all, t_all, f_all / t_all
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
