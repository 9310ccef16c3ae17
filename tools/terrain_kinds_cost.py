#!/usr/bin/env python3
"""`python bench.py --terrain trimesh` on the course of all tile kinds: the benchmark as it is, with the Go2 config's
`terrain.terrain_proportions` set first (bench.py has no flag for it).  Prints bench.py's JSON line; compare with the same command without
this wrapper (the two-kind course, profiles/r6_final_bench_cfg2_trimesh.json) for what risers and holes cost the height-field step.

  python tools/terrain_kinds_cost.py [--proportions 0.1,0.1,0.35,0.25,0.2] [--curriculum] [bench.py's flags, e.g. --steps 20 --warmup 5]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    props = "0.1,0.1,0.35,0.25,0.2"
    if "--proportions" in argv:
        i = argv.index("--proportions")
        props = argv[i + 1]
        del argv[i:i + 2]
    curriculum = "--curriculum" in argv
    if curriculum:
        argv.remove("--curriculum")
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    Go2LocomotionCfg.terrain.terrain_proportions = [float(x) for x in props.split(",")]
    Go2LocomotionCfg.terrain.curriculum = curriculum
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--terrain", "trimesh"] + argv
    bench.main()


if __name__ == "__main__":
    main()
