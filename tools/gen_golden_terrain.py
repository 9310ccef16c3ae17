#!/usr/bin/env python3
"""Generate tests/golden/terrain_kinds.npz by RUNNING THE REFERENCE'S OWN `Terrain.make_terrain`, `gap_terrain`, `pit_terrain` and
`add_terrain_to_map` (bbc/legged_gym/utils/terrain.py:81-164) on CPU (the recipe of tools/gen_golden.py, whose `import_reference`
this uses; build container only).

isaacgym.terrain_utils is an empty module in tools/ref_shims, so the five generators the ladder takes from it are RECORDING STUBS here:
each notes its name and arguments and writes nothing.  The reference's own gap_terrain / pit_terrain are wrapped the same way and
still run.  The file holds arrays and one name table only:

  names                  the seven generators, "name:param,param,..." in the order the argument vectors use
  choices, difficulties  the grid
  props5, props7         the two terrain_proportions lists
  calls5, calls7         (choice, difficulty, 2, 1 + 5): per grid point up to two calls [index into names | arguments], NaN where
                         there is no call or the reference passed no value (a default)
  tile_difficulties      three difficulties
  gap_tiles, pit_tiles   (3, 100, 100) int16: what the reference's two functions wrote at gap_size = pit depth = difficulty
  map_raw, env_origins   those six tiles in a 2 x 3 map behind a 3 m border, and add_terrain_to_map's origins
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import GOLD, import_reference  # noqa: E402

PARAMS = {
    "pyramid_sloped_terrain": ("slope", "platform_size"),
    "random_uniform_terrain": ("min_height", "max_height", "step", "downsampled_scale"),
    "pyramid_stairs_terrain": ("step_width", "step_height", "platform_size"),
    "discrete_obstacles_terrain": ("max_height", "min_size", "max_size", "num_rects", "platform_size"),
    "stepping_stones_terrain": ("stone_size", "stone_distance", "max_height", "platform_size", "depth"),
    "gap_terrain": ("gap_size", "platform_size"),
    "pit_terrain": ("depth", "platform_size"),
}
NAMES = list(PARAMS)
WIDTH = 1 + max(len(v) for v in PARAMS.values())
CHOICES = np.round(np.arange(40) / 40 + 0.001, 6)            # 0.001 .. 0.976: both sides of every cumulative share below
DIFFICULTIES = np.array([0.0, 0.25, 0.5, 0.9])
PROPS5 = [0.1, 0.1, 0.35, 0.25, 0.2]
PROPS7 = [0.1, 0.1, 0.15, 0.15, 0.1, 0.15, 0.15]             # sums to 0.9: the rest are pits
TILE_DIFFICULTIES = np.array([0.25, 0.5, 0.9])
HSCALE, VSCALE, TILE = 0.1, 0.005, 100


class Recorder:
    """stands in for a generator: notes (name, arguments by parameter name) and, if it wraps one, runs it"""

    def __init__(self, log, name, inner=None):
        self.log, self.name, self.inner = log, name, inner

    def __call__(self, terrain, *args, **kwargs):
        row = np.full(WIDTH, np.nan)
        row[0] = NAMES.index(self.name)
        given = dict(zip(PARAMS[self.name], args))
        assert not set(given) & set(kwargs) and set(kwargs) <= set(PARAMS[self.name]), (self.name, args, kwargs)
        given.update(kwargs)
        for k, v in given.items():
            row[1 + PARAMS[self.name].index(k)] = v
        self.log.append(row)
        if self.inner is not None:
            return self.inner(terrain, *args, **kwargs)
        return terrain


class StubSubTerrain:
    def __init__(self, terrain_name="terrain", width=256, length=256, vertical_scale=1.0, horizontal_scale=1.0):
        self.terrain_name, self.width, self.length = terrain_name, width, length
        self.vertical_scale, self.horizontal_scale = vertical_scale, horizontal_scale
        self.height_field_raw = np.zeros((width, length), dtype=np.int16)


def ladder(make_terrain, owner, log, props):
    """calls[choice, difficulty, slot] of `make_terrain` (bound to `owner`, whose cumulative shares are set here) over the grid"""
    owner.proportions = [np.sum(props[:i + 1]) for i in range(len(props))]
    out = np.full((len(CHOICES), len(DIFFICULTIES), 2, WIDTH), np.nan)
    for a, choice in enumerate(CHOICES):
        for b, difficulty in enumerate(DIFFICULTIES):
            del log[:]
            make_terrain(float(choice), float(difficulty))
            assert 1 <= len(log) <= 2, (choice, difficulty, log)
            for s, row in enumerate(log):
                out[a, b, s] = row
    return out


def main():
    import_reference()
    import isaacgym
    import legged_gym.utils.terrain as ref
    log = []
    tu = isaacgym.terrain_utils
    tu.SubTerrain = StubSubTerrain
    for name in NAMES[:5]:
        setattr(tu, name, Recorder(log, name))
    ref_gap, ref_pit = ref.gap_terrain, ref.pit_terrain
    ref.gap_terrain, ref.pit_terrain = Recorder(log, "gap_terrain", ref_gap), Recorder(log, "pit_terrain", ref_pit)

    import types
    t = object.__new__(ref.Terrain)
    t.cfg = types.SimpleNamespace(vertical_scale=VSCALE, horizontal_scale=HSCALE)
    t.width_per_env_pixels = t.length_per_env_pixels = TILE
    out = dict(names=np.array([n + ":" + ",".join(PARAMS[n]) for n in NAMES]), choices=CHOICES, difficulties=DIFFICULTIES,
               props5=np.array(PROPS5), props7=np.array(PROPS7), tile_difficulties=TILE_DIFFICULTIES)
    out["calls5"] = ladder(t.make_terrain, t, log, PROPS5)
    out["calls7"] = ladder(t.make_terrain, t, log, PROPS7)
    for key in ("calls5", "calls7"):
        ran = {NAMES[int(i)] for i in out[key][..., 0].ravel() if not np.isnan(i)}
        print(key, "ran", sorted(ran))
    assert {NAMES[int(i)] for i in out["calls7"][..., 0].ravel() if not np.isnan(i)} == set(NAMES)

    # the reference's own two generators, and add_terrain_to_map on their tiles
    t.env_length = t.env_width = TILE * HSCALE
    t.border = int(3.0 / HSCALE)
    t.height_field_raw = np.zeros((2 * TILE + 2 * t.border, 3 * TILE + 2 * t.border), dtype=np.int16)
    t.env_origins = np.zeros((2, 3, 3))
    gaps, pits = [], []
    for k, d in enumerate(TILE_DIFFICULTIES):
        g = StubSubTerrain(width=TILE, length=TILE, vertical_scale=VSCALE, horizontal_scale=HSCALE)
        ref_gap(g, gap_size=float(d), platform_size=3.0)
        p = StubSubTerrain(width=TILE, length=TILE, vertical_scale=VSCALE, horizontal_scale=HSCALE)
        ref_pit(p, depth=float(d), platform_size=4.0)
        t.add_terrain_to_map(g, 0, k); t.add_terrain_to_map(p, 1, k)
        gaps.append(g.height_field_raw.copy()); pits.append(p.height_field_raw.copy())
    out["gap_tiles"], out["pit_tiles"] = np.stack(gaps), np.stack(pits)
    out["map_raw"], out["env_origins"] = t.height_field_raw, t.env_origins
    assert out["gap_tiles"].dtype == np.int16 and out["gap_tiles"].min() == -1000 and out["pit_tiles"].min() == -int(0.9 / VSCALE)
    path = os.path.join(GOLD, "terrain_kinds.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; origins z {out['env_origins'][..., 2].tolist()}")


if __name__ == "__main__":
    main()
