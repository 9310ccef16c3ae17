#!/usr/bin/env python3
"""Generate tests/golden/terrain_curriculum.npz by RUNNING THE REFERENCE'S OWN `_update_terrain_curriculum`
(bbc/legged_gym/envs/base/legged_robot.py:689-711) on CPU, as an unbound method on a stub (the recipe of tools/gen_golden.py,
whose `import_reference` this uses; build container only).

The file holds arrays only: the inputs (`root_states`, `env_origins`, `commands`, `terrain_levels`, `terrain_types`,
`terrain_origins`, `env_length`, `max_episode_length_s`, `env_ids`) and the reference's outputs (`out_terrain_levels`,
`out_env_origins`, all envs; only `env_ids` may differ from the inputs).  `graduated` (this tool's restatement of the move-up test, not a reference output) marks the envs of `env_ids` that moved past
the last row: the reference redraws their level with torch.randint_like, which a counter-based Philox cannot reproduce, so a test
compares them by property (level in [0, rows), origin = table[level, type]) and everything else exactly.

Inputs are constructed, not sampled near the thresholds: every distance is at least 1e-3 away from env_length / 2 and from
|commands[:2]| * max_episode_length_s * 0.5, so that a rounding difference in a square root cannot flip a decision.
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import GOLD, import_reference  # noqa: E402

N, ROWS, COLS = 240, 4, 3
ENV_LENGTH, EPISODE_S = 8.0, 20.0
MARGIN = 1e-3


def make_inputs(seed=7):
    rng = np.random.default_rng(seed)
    origins = np.zeros((ROWS, COLS, 3), np.float32)
    for r in range(ROWS):
        for c in range(COLS):
            origins[r, c] = [(r + 0.5) * ENV_LENGTH + 0.125 * c, (c + 0.5) * ENV_LENGTH + 0.25 * r, 0.03125 * (1 + r * COLS + c)]
    levels = rng.integers(0, ROWS, N).astype(np.int64)
    levels[:40] = ROWS - 1                                   # enough envs on the top row to graduate
    levels[40:80] = 0                                        # ... and on the bottom row to be floored
    types_ = rng.integers(0, COLS, N).astype(np.int64)
    env_origins = origins[levels, types_].copy()
    # commanded speed, and the walked distance as a fraction of what decides: 3 classes (up / down / stay), cycled over the envs
    speed = rng.uniform(0.1, 0.75, N).astype(np.float32)     # |cmd| * 20 s * 0.5 in [1, 7.5] m: below env_length / 2 = 4 m for some, above for others
    speed[rng.random(N) < 0.15] = 0.0                        # standing commands: never "down"
    heading = rng.uniform(-np.pi, np.pi, N)
    commands = np.zeros((N, 5), np.float32)
    commands[:, 0] = speed * np.cos(heading); commands[:, 1] = speed * np.sin(heading)
    need = np.linalg.norm(commands[:, :2].astype(np.float64), axis=1) * EPISODE_S * 0.5
    half = ENV_LENGTH / 2
    dist = np.zeros(N)
    for i in range(N):
        k = i % 3
        for _ in range(1000):     # redraw until the distance is clear of BOTH thresholds (an "up" env's distance can fall next to the one for "down")
            lo = min(need[i], half)
            if k == 0:                      # up
                dist[i] = rng.uniform(half + 0.01, half + 3.0)
            elif k == 1 and lo > 0.05:      # down (a standing command cannot go down: it takes the last branch)
                dist[i] = rng.uniform(0.0, lo - 0.01)
            elif lo + 0.05 < half:          # between the two thresholds: stay
                dist[i] = rng.uniform(lo + 0.01, half - 0.01)
            else:                           # no room between them: anywhere below
                dist[i] = rng.uniform(0.0, half - 0.01)
            if abs(dist[i] - half) >= 5 * MARGIN and abs(dist[i] - need[i]) >= 5 * MARGIN:
                break
        else:
            raise RuntimeError(f"no distance clear of both thresholds for env {i}")
    ang = rng.uniform(-np.pi, np.pi, N)
    root = np.zeros((N, 13), np.float32)                    # the update reads columns 0:2 only; z is set for a plausible pose, the rest stays 0
    root[:, 0] = env_origins[:, 0] + (dist * np.cos(ang)).astype(np.float32)
    root[:, 1] = env_origins[:, 1] + (dist * np.sin(ang)).astype(np.float32)
    root[:, 2] = env_origins[:, 2] + 0.3
    env_ids = np.sort(rng.choice(N, size=(2 * N) // 3, replace=False)).astype(np.int64)
    # the margin the docstring promises, on the fp32 values the reference will see
    d32 = np.linalg.norm((root[:, :2] - env_origins[:, :2]).astype(np.float64), axis=1)
    need32 = np.linalg.norm(commands[:, :2].astype(np.float64), axis=1) * EPISODE_S * 0.5
    assert (np.abs(d32 - half) >= MARGIN).all() and (np.abs(d32 - need32) >= MARGIN).all()
    return dict(root_states=root, env_origins=env_origins, commands=commands, terrain_levels=levels, terrain_types=types_, terrain_origins=origins,
                env_length=np.float32(ENV_LENGTH), max_episode_length_s=np.float32(EPISODE_S), env_ids=env_ids)


def main():
    ref_lr, _, _ = import_reference()
    inp = make_inputs()
    env = object.__new__(ref_lr.LeggedRobot)
    env.init_done = True
    env.root_states = torch.from_numpy(inp["root_states"].copy())
    env.env_origins = torch.from_numpy(inp["env_origins"].copy())
    env.commands = torch.from_numpy(inp["commands"].copy())
    env.terrain_levels = torch.from_numpy(inp["terrain_levels"].copy())
    env.terrain_types = torch.from_numpy(inp["terrain_types"].copy())
    env.terrain_origins = torch.from_numpy(inp["terrain_origins"].copy())
    env.terrain = types.SimpleNamespace(env_length=float(inp["env_length"]))
    env.max_episode_length_s = float(inp["max_episode_length_s"])
    env.max_terrain_level = ROWS
    ids = torch.from_numpy(inp["env_ids"].copy())
    torch.manual_seed(0)
    ref_lr.LeggedRobot._update_terrain_curriculum(env, ids)
    # which envs graduated: THIS TOOL'S restatement of the move-up test on the inputs (the reference's run leaves no trace of it once the level is
    # redrawn); the margins above keep the restatement and the reference on the same side of the threshold
    d = torch.norm(torch.from_numpy(inp["root_states"])[ids, :2] - torch.from_numpy(inp["env_origins"])[ids, :2], dim=1)
    graduated = ((torch.from_numpy(inp["terrain_levels"])[ids] == ROWS - 1) & (d > float(inp["env_length"]) / 2)).numpy()
    out = dict(inp)
    out["out_terrain_levels"] = env.terrain_levels.numpy().astype(np.int64)
    out["out_env_origins"] = env.env_origins.numpy().astype(np.float32)
    out["graduated"] = graduated
    assert graduated.sum() >= 8 and (~graduated).sum() > 100
    lv = out["out_terrain_levels"]
    assert lv.min() >= 0 and lv.max() < ROWS
    path = os.path.join(GOLD, "terrain_curriculum.npz")
    np.savez_compressed(path, **out)
    moved = lv[inp["env_ids"]] - inp["terrain_levels"][inp["env_ids"]]
    print(f"wrote {path}: {os.path.getsize(path)} bytes; of {len(ids)} resetting envs {int((moved > 0).sum())} up, {int((moved < 0).sum())} down (or redrawn lower), "
          f"{int((moved == 0).sum())} unchanged, {int(graduated.sum())} graduated")


if __name__ == "__main__":
    main()
