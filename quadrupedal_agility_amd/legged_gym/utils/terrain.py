"""Terrain tiles for the BBC task (API of bbc/legged_gym/utils/terrain.py:9-164).

The reference builds a 10 x 10 grid of 10 m tiles with isaacgym.terrain_utils generators and hands the
int16 height field (or its triangulation) to PhysX.  Here the same int16 field goes into the engine's
HEIGHT_SAMPLES tensor (include/qa_sim.h).  All seven tile kinds of the reference's `make_terrain` ladder
are built: smooth and rough pyramid slopes, pyramid stairs (up and down), discrete obstacles, stepping
stones, gaps and pits; `terrain.selected` builds every tile with one named generator.

'heightfield' and 'trimesh' are the same surface in this build: two triangles per cell.  On the two slope
tiles (under 0.16) that is also what the reference has, because its trimesh slope-threshold correction
does not trigger below `slope_treshold` = 0.75 (on the Go2 course only a few cells of the seams between
two rough tiles exceed it, about 0.01 % of the map).  On risers, block edges, stone edges and rims it does
trigger: the reference's mesh gets vertical faces there, this build keeps the one-cell ramp of the
reference's own 'heightfield' mode.  A 'trimesh' map with such cells logs one warning
that names their share; a smaller `horizontal_scale` narrows the ramps (the engine takes any scale).

Random draws use numpy's global RNG like the reference (seeded by set_seed), in the reference's order,
so tile layouts are distribution-, not bit-compatible (isaacgym.terrain_utils is not available to
compare against)."""
import logging

import numpy as np
from scipy.interpolate import RegularGridInterpolator


class SubTerrain:
    def __init__(self, terrain_name="terrain", width=256, length=256, vertical_scale=1.0, horizontal_scale=1.0):
        self.terrain_name = terrain_name
        self.vertical_scale, self.horizontal_scale = vertical_scale, horizontal_scale
        self.width, self.length = width, length
        self.height_field_raw = np.zeros((width, length), dtype=np.int16)


def pyramid_sloped_terrain(terrain, slope=1.0, platform_size=1.0):
    """Pyramid rising (slope > 0) or sinking (slope < 0) towards the tile centre, cut off by a flat platform."""
    cx, cy = terrain.width // 2, terrain.length // 2
    fx = ((cx - np.abs(cx - np.arange(terrain.width))) / cx).reshape(terrain.width, 1)
    fy = ((cy - np.abs(cy - np.arange(terrain.length))) / cy).reshape(1, terrain.length)
    peak = int(slope * (terrain.horizontal_scale / terrain.vertical_scale) * (terrain.width / 2))
    terrain.height_field_raw += (peak * fx * fy).astype(terrain.height_field_raw.dtype)
    half = int(platform_size / terrain.horizontal_scale / 2)
    edge = terrain.height_field_raw[cx - half, cy - half]
    terrain.height_field_raw = np.clip(terrain.height_field_raw, min(edge, 0), max(edge, 0))
    return terrain


def random_uniform_terrain(terrain, min_height, max_height, step=1.0, downsampled_scale=None):
    """Heights drawn from {min, min+step, ..., max} on a coarse grid, bilinearly upsampled and ADDED to the tile."""
    ds = terrain.horizontal_scale if downsampled_scale is None else downsampled_scale
    lo, hi, st = int(min_height / terrain.vertical_scale), int(max_height / terrain.vertical_scale), int(step / terrain.vertical_scale)
    levels = np.arange(lo, hi + st, st)
    nx = int(terrain.width * terrain.horizontal_scale / ds)
    ny = int(terrain.length * terrain.horizontal_scale / ds)
    coarse = np.random.choice(levels, (nx, ny))
    x = np.linspace(0, terrain.width * terrain.horizontal_scale, nx)
    y = np.linspace(0, terrain.length * terrain.horizontal_scale, ny)
    f = RegularGridInterpolator((x, y), coarse.astype(np.float64), method="linear")
    xu = np.linspace(0, terrain.width * terrain.horizontal_scale, terrain.width)
    yu = np.linspace(0, terrain.length * terrain.horizontal_scale, terrain.length)
    gx, gy = np.meshgrid(xu, yu, indexing="ij")
    terrain.height_field_raw += np.rint(f(np.stack([gx, gy], axis=-1))).astype(np.int16)
    return terrain


def _zero_platform(terrain, cells):
    """the central `cells` x `cells` square back to height 0"""
    x1, x2 = (terrain.width - cells) // 2, (terrain.width + cells) // 2
    y1, y2 = (terrain.length - cells) // 2, (terrain.length + cells) // 2
    terrain.height_field_raw[x1:x2, y1:y2] = 0


def pyramid_stairs_terrain(terrain, step_width, step_height, platform_size=1.0):
    """Concentric square steps rising (step_height > 0) or sinking (< 0) towards the tile centre.  The window shrinks by
    one step width per side until an extent is no larger than the platform, so the top is platform_size minus at most two
    step widths wide."""
    sw, sh = int(step_width / terrain.horizontal_scale), int(step_height / terrain.vertical_scale)
    plat = int(platform_size / terrain.horizontal_scale)
    if sw < 1:
        raise ValueError(f"pyramid_stairs_terrain: step_width {step_width} is less than one cell of {terrain.horizontal_scale} m")
    x0, x1, y0, y1, h = 0, terrain.width, 0, terrain.length, 0
    while x1 - x0 > plat and y1 - y0 > plat:
        x0 += sw; x1 -= sw; y0 += sw; y1 -= sw
        h += sh
        terrain.height_field_raw[x0:x1, y0:y1] = h
    return terrain


def discrete_obstacles_terrain(terrain, max_height, min_size, max_size, num_rects, platform_size=1.0):
    """`num_rects` rectangular blocks and holes of height +-H or +-H // 2 at random places (later ones overwrite earlier ones),
    around a flat central platform.  Per rectangle the draws are: width, length, start_i, start_j, height."""
    H = int(max_height / terrain.vertical_scale)
    lo, hi = int(min_size / terrain.horizontal_scale), int(max_size / terrain.horizontal_scale)
    rows, cols = terrain.height_field_raw.shape
    heights = [-H, -H // 2, H // 2, H]
    sizes = range(lo, hi, 4)
    for _ in range(num_rects):
        w = np.random.choice(sizes)
        l = np.random.choice(sizes)
        i = np.random.choice(range(0, rows - w, 4))
        j = np.random.choice(range(0, cols - l, 4))
        terrain.height_field_raw[i:i + w, j:j + l] = np.random.choice(heights)
    _zero_platform(terrain, int(platform_size / terrain.horizontal_scale))
    return terrain


def stepping_stones_terrain(terrain, stone_size, stone_distance, max_height, platform_size=1.0, depth=-10):
    """Square stones `stone_size` wide, `stone_distance` apart, over a floor at `depth`; every row of stones starts at a random
    offset, and each stone's height is one draw from [-max_height - 1, max_height) raw units.  The walk goes row by row along y
    (along x when the tile is wider than long)."""
    size, dist = int(stone_size / terrain.horizontal_scale), int(stone_distance / terrain.horizontal_scale)
    if size < 1:
        raise ValueError(f"stepping_stones_terrain: stone_size {stone_size} is less than one cell of {terrain.horizontal_scale} m")
    mh = int(max_height / terrain.vertical_scale)
    height_range = np.arange(-mh - 1, mh, 1)
    transposed = terrain.width > terrain.length
    hf = terrain.height_field_raw.T if transposed else terrain.height_field_raw       # a view: hf[along the row, across rows]
    hf[:, :] = int(depth / terrain.vertical_scale)
    n_along, n_across = hf.shape
    b = 0
    while b < n_across:
        b1 = min(n_across, b + size)
        a = np.random.randint(0, size)
        hf[0:max(0, a - dist), b:b1] = np.random.choice(height_range)                 # the piece in front of the first stone
        while a < n_along:
            hf[a:min(n_along, a + size), b:b1] = np.random.choice(height_range)
            a += size + dist
        b += size + dist
    _zero_platform(terrain, int(platform_size / terrain.horizontal_scale))
    return terrain


def gap_terrain(terrain, gap_size, platform_size=1.0):
    """A square moat of 5 m depth (-1000 raw, whatever the vertical scale: the reference's constant) around a central island.
    The reference measures both squares as HALF extents from the centre: the island is (tile - platform_size) wide, the moat
    `gap_size` wide beyond it (terrain.py:142-154)."""
    gap, plat = int(gap_size / terrain.horizontal_scale), int(platform_size / terrain.horizontal_scale)
    cx, cy = terrain.length // 2, terrain.width // 2
    ix, iy = (terrain.length - plat) // 2, (terrain.width - plat) // 2                # island half extents
    ox, oy = ix + gap, iy + gap                                                       # moat outer half extents
    terrain.height_field_raw[cx - ox:cx + ox, cy - oy:cy + oy] = -1000
    terrain.height_field_raw[cx - ix:cx + ix, cy - iy:cy + iy] = 0


def pit_terrain(terrain, depth, platform_size=1.0):
    """A central square pit, `depth` below the tile (terrain.py:157-164)."""
    d, half = int(depth / terrain.vertical_scale), int(platform_size / terrain.horizontal_scale / 2)
    cx, cy = terrain.length // 2, terrain.width // 2
    terrain.height_field_raw[cx - half:cx + half, cy - half:cy + half] = -d


GENERATORS = {f.__name__: f for f in (pyramid_sloped_terrain, random_uniform_terrain, pyramid_stairs_terrain, discrete_obstacles_terrain,
                                      stepping_stones_terrain, gap_terrain, pit_terrain)}


class Terrain:
    def __init__(self, cfg, num_robots):
        self.cfg, self.num_robots, self.type = cfg, num_robots, cfg.mesh_type
        if self.type in ["none", "plane", None]:
            return
        self.env_length, self.env_width = cfg.terrain_length, cfg.terrain_width
        uses_ladder = cfg.curriculum or not cfg.selected                      # terrain.selected alone does not read the list
        if uses_ladder and (not 5 <= len(cfg.terrain_proportions) <= 7 or any(p < 0 for p in cfg.terrain_proportions)):
            raise ValueError(f"terrain_proportions {list(cfg.terrain_proportions)}: five to seven non-negative shares (smooth slope, rough slope, "
                             "stairs down, stairs up, discrete obstacles[, stepping stones[, gaps]]; the rest are pits)")
        self.proportions = [np.sum(cfg.terrain_proportions[:i + 1]) for i in range(len(cfg.terrain_proportions))]
        cfg.num_sub_terrains = cfg.num_rows * cfg.num_cols
        self.env_origins = np.zeros((cfg.num_rows, cfg.num_cols, 3))
        self.width_per_env_pixels = int(self.env_width / cfg.horizontal_scale)
        self.length_per_env_pixels = int(self.env_length / cfg.horizontal_scale)
        self.border = int(cfg.border_size / cfg.horizontal_scale)
        self.tot_cols = int(cfg.num_cols * self.width_per_env_pixels) + 2 * self.border
        self.tot_rows = int(cfg.num_rows * self.length_per_env_pixels) + 2 * self.border
        self.height_field_raw = np.zeros((self.tot_rows, self.tot_cols), dtype=np.int16)
        self.difficulties = cfg.difficulties
        if cfg.curriculum:
            for j in range(cfg.num_cols):
                for i in range(cfg.num_rows):
                    self.add_terrain_to_map(self.make_terrain(j / cfg.num_cols + 0.001, i / cfg.num_rows), i, j)
        elif cfg.selected:
            self.selected_terrain()
        else:
            for k in range(cfg.num_sub_terrains):
                i, j = np.unravel_index(k, (cfg.num_rows, cfg.num_cols))
                choice = np.random.uniform(0, 1)
                difficulty = np.random.choice(self.difficulties)
                self.add_terrain_to_map(self.make_terrain(choice, difficulty), i, j)
        self.heightsamples = self.height_field_raw
        if self.type == "trimesh":
            share = self.steep_cell_share()
            if share > 0:
                logging.getLogger(__name__).warning(
                    "terrain: %.2f %% of the map's cells are steeper than slope_treshold = %g; the reference's trimesh has vertical faces there, "
                    "this build a ramp one cell (%g m) wide, as the reference's 'heightfield' mode has.  A smaller terrain.horizontal_scale narrows the ramps.  "
                    "(On a course of slope tiles only, a share around 0.01 %% is the seams between two rough tiles and nothing else.)",
                    100.0 * share, cfg.slope_treshold, cfg.horizontal_scale)

    def steep_cell_share(self):
        """share of the map's cells with a rise along x or y above slope_treshold: where the reference's trimesh conversion moves vertices"""
        h = self.height_field_raw.astype(np.int32)
        limit = self.cfg.slope_treshold * self.cfg.horizontal_scale / self.cfg.vertical_scale
        dx, dy = np.abs(np.diff(h, axis=0))[:, :-1], np.abs(np.diff(h, axis=1))[:-1, :]
        return float(np.mean(np.maximum(dx, dy) > limit))

    def _sub_terrain(self):
        return SubTerrain("terrain", width=self.width_per_env_pixels, length=self.width_per_env_pixels,
                          vertical_scale=self.cfg.vertical_scale, horizontal_scale=self.cfg.horizontal_scale)

    def selected_terrain(self):
        """terrain.selected: every tile from the generator terrain_kwargs["type"] names (terrain.py:66-79).  The name is looked up, not
        evaluated; the arguments are the dict's other entries or its nested "terrain_kwargs"; the config's dict is left as it is."""
        kw = dict(self.cfg.terrain_kwargs or {})
        name = kw.pop("type", None)
        key = name[len("terrain_utils."):] if isinstance(name, str) and name.startswith("terrain_utils.") else name
        if key not in GENERATORS:
            raise ValueError(f"terrain.terrain_kwargs['type'] = {name!r}: expected one of {', '.join(GENERATORS)}")
        if "terrain_kwargs" in kw:
            if len(kw) > 1:
                raise ValueError("terrain.terrain_kwargs: either a nested 'terrain_kwargs' dict or the generator's arguments beside 'type', not both")
            kw = dict(kw["terrain_kwargs"] or {})
        for k in range(self.cfg.num_sub_terrains):
            i, j = np.unravel_index(k, (self.cfg.num_rows, self.cfg.num_cols))
            t = self._sub_terrain()
            GENERATORS[key](t, **kw)
            self.add_terrain_to_map(t, i, j)

    def make_terrain(self, choice, difficulty):
        t = self._sub_terrain()
        # cumulative shares of the seven branches: a missing entry has zero share, what lies beyond the last goes to the pits
        p = list(self.proportions) + [self.proportions[-1] if self.proportions else 0.0] * (7 - len(self.proportions))
        slope = difficulty * 0.4
        step_height = 0.05 + 0.18 * difficulty
        discrete_obstacles_height = 0.05 + difficulty * 0.2
        stepping_stones_size = 1.5 * (1.05 - difficulty)
        stone_distance = 0.05 if difficulty == 0 else 0.1
        gap_size = pit_depth = 1.0 * difficulty
        if choice < p[0]:
            if choice < p[0] / 2:
                slope *= -1
            pyramid_sloped_terrain(t, slope=slope, platform_size=3.0)
        elif choice < p[1]:
            pyramid_sloped_terrain(t, slope=slope, platform_size=3.0)
            random_uniform_terrain(t, min_height=-0.05, max_height=0.05, step=0.005, downsampled_scale=0.2)
        elif choice < p[3]:
            if choice < p[2]:
                step_height *= -1
            pyramid_stairs_terrain(t, step_width=0.31, step_height=step_height, platform_size=3.0)
        elif choice < p[4]:
            discrete_obstacles_terrain(t, discrete_obstacles_height, 1.0, 2.0, 20, platform_size=3.0)
        elif choice < p[5]:
            stepping_stones_terrain(t, stone_size=stepping_stones_size, stone_distance=stone_distance, max_height=0.0, platform_size=4.0)
        elif choice < p[6]:
            gap_terrain(t, gap_size=gap_size, platform_size=3.0)
        else:
            pit_terrain(t, depth=pit_depth, platform_size=4.0)
        return t

    def add_terrain_to_map(self, terrain, row, col):
        sx, sy = self.border + row * self.length_per_env_pixels, self.border + col * self.width_per_env_pixels
        self.height_field_raw[sx:sx + self.length_per_env_pixels, sy:sy + self.width_per_env_pixels] = terrain.height_field_raw
        hs = terrain.horizontal_scale
        x1, x2 = int((self.env_length / 2.0 - 1) / hs), int((self.env_length / 2.0 + 1) / hs)
        y1, y2 = int((self.env_width / 2.0 - 1) / hs), int((self.env_width / 2.0 + 1) / hs)
        z = np.max(terrain.height_field_raw[x1:x2, y1:y2]) * terrain.vertical_scale
        self.env_origins[row, col] = [(row + 0.5) * self.env_length, (col + 0.5) * self.env_width, z]
