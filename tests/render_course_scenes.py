"""Scenes of the course renderer shared by tests/test_render_course_cpu.py (the reference alone, and the host twin against it) and
tests/test_render_course.py (the kernel against the reference).  Like tests/render_scenes.py every number is representable in fp32.  The
references are computed once per process (`reference`)."""
import functools

import numpy as np

from tests import render_course_ref as rc
from tests import render_ref as rr
from tests import render_scenes as rs

W, H = 96, 64
SEESAW, BAR, TYRE = 1.0, 2.0, 3.0           # QA_OBST_*
MAX_TILT = float(np.float32(0.16744808))    # QA_SEESAW_MAX_TILT
YAW = 0.6
LIGHT = (0.35, 0.25, 1.0)


def _desc(x, y, yaw, hl, hw, h0, kind):
    return [x, y, np.cos(yaw), np.sin(yaw), hl, hw, h0, kind]


def _state(q):
    return [q, 0.0, 0.0, 1.0]


def _scene(bs, env_ids, cams, hm, cm=None, far=9.0, width=W, height=H, **course):
    s = dict(body_state=rs._f32(bs), env_ids=list(env_ids), cameras=rs._f32(np.stack(cams)), width=width, height=height, far=far,
             light_dir=rs._f32(LIGHT), flags=3, terrain=rs._terrain(hm, cm))
    s.update({k: (rs._f32(v) if k in ("obst_desc", "obst_state", "goals") else v) for k, v in course.items()})
    return s


SEESAW_AT = (4.0, 4.0)


def seesaw_scene(width=W, height=H):
    """the see-saw at +stop (env 0), -stop (env 1) and 0.05 (env 2), its footprint turned by 0.6 so that it cuts the cells obliquely, over a
    map that holds a static A-frame there (which the drawn surface ignores, as the physics does).  Camera 0 / 2: above the plank of envs 0 /
    1; camera 1 / 3: beside the plank of envs 0 / 2, below its high end -- the long side face.  Every env is a decoy for the others: same
    footprint, another tilt."""
    hm = np.zeros((rs.ROWS, rs.COLS), np.int16)
    i, j = np.meshgrid(np.arange(rs.ROWS), np.arange(rs.COLS), indexing="ij")
    x, y = i * rs.HS - rs.BORDER - SEESAW_AT[0], j * rs.HS - rs.BORDER - SEESAW_AT[1]
    lx, ly = np.cos(YAW) * x + np.sin(YAW) * y, np.cos(YAW) * y - np.sin(YAW) * x
    frame = (np.abs(lx) <= 1.3) & (np.abs(ly) <= 0.2)
    hm[frame] = np.round((0.26 * (1 - np.abs(lx[frame]) / 1.5)) / rs.VS).astype(np.int16)
    desc = np.zeros((3, 3, 8)); state = np.zeros((3, 3, 4))
    for e, q in enumerate((MAX_TILT, -MAX_TILT, 0.05)):
        desc[e, 0] = _desc(*SEESAW_AT, YAW, 1.5, 0.3, 0.26, SEESAW)
        state[e, 0] = _state(q)
    bs = np.stack([rr.standing_body_state(root=(5.6, 2.9, 0.33), yaw=0.3 * e) for e in range(3)])
    ax = np.array([np.cos(YAW), np.sin(YAW), 0.0]); ay = np.array([-np.sin(YAW), np.cos(YAW), 0.0]); c = np.array(SEESAW_AT + (0.0,))
    cams = [rs.camera(c + (0.37, -2.93, 2.41), c + (0.1, 0.0, 0.2), 50.0),
            rs.camera(c - 1.1 * ax - 1.83 * ay + (0, 0, 0.31), c - 1.1 * ax + (0, 0, 0.3), 55.0),        # +stop: lx < 0 is the high end
            rs.camera(c + (-0.39, -2.77, 2.19), c + (0.13, 0.07, 0.2), 47.0),
            rs.camera(c - 0.9 * ax + 1.79 * ay + (0, 0, 0.27), c - 0.7 * ax + (0, 0, 0.25), 55.0)]
    return _scene(bs, [0, 0, 1, 2], cams, hm, obst_desc=desc, obst_state=state)


def bar_tyre_scene(width=W, height=H):
    """a jump bar raised by q = +0.05 and a tyre lowered by q = -0.05 (floor cells and ceiling triangles move together), and a slot of kind
    0 over a raised block that must stay as the map has it; env 1 is the decoy (other offsets)"""
    hm = np.zeros((rs.ROWS, rs.COLS), np.int16); cm = np.full((rs.ROWS, rs.COLS), rr.NO_CEILING, np.int16)
    hm[20:22, 16:26] = 60                       # the bar: x 3.0 .. 3.25, y 2.0 .. 4.25, 0.3 m
    hm[31:34, 19:24] = 40                       # the tyre's lower rim, 0.2 m ...
    cm[31:34, 19:24] = 160                      # ... and the ring's upper part, from 0.8 m
    hm[26:28, 8:12] = 80                        # a block under the empty slot
    desc = np.zeros((3, 3, 8)); state = np.zeros((3, 3, 4))
    for e, (qb, qt) in enumerate(((0.05, -0.05), (-0.12, 0.15), (0.0, 0.0))):
        desc[e, 0] = _desc(4.6, 0.3, 0.3, 0.6, 0.5, 0.0, 0.0); state[e, 0] = _state(0.2)           # kind 0: ignored
        desc[e, 1] = _desc(3.11, 3.07, 0.0, 0.33, 1.21, 0.0, BAR); state[e, 1] = _state(qb)
        desc[e, 2] = _desc(6.12, 3.36, 0.0, 0.43, 0.71, 0.0, TYRE); state[e, 2] = _state(qt)
    bs = np.stack([rr.standing_body_state(root=(4.6, 3.1, 0.33), yaw=0.2)] * 3)
    cams = [rs.camera((0.83, 1.47, 1.53), (4.0, 3.0, 0.2), 55.0), rs.camera((7.63, 2.11, 0.33), (6.0, 3.3, 0.9), 55.0)]
    return _scene(bs, [0, 0], cams, hm, cm, obst_desc=desc, obst_state=state, width=width, height=height)


NUM_GOALS = 26


def goals_scene():
    """goals alone (no records) over the tilted map of render_scenes: one in front of the robot, one behind it, one half sunk into the
    floor; 26 rows per env, the unused ones repeating the last goal; env 0's current goal is 0, env 1's is 1 and reached, env 2's is 2"""
    x, y = 4.0, 4.6
    bs = np.stack([rr.standing_body_state(root=(x, y, 0.34 + rs.tilted_height(x, y)), yaw=-0.5)] * 3)
    g = np.zeros((3, NUM_GOALS, 3))
    pts = [(3.3, 3.9, rs.tilted_height(3.3, 3.9) + 0.35), (4.6, 5.3, rs.tilted_height(4.6, 5.3) + 0.3), (3.1, 5.2, rs.tilted_height(3.1, 5.2))]
    for e in range(3):
        g[e, :3] = pts; g[e, 3:] = pts[2]
    cams = [rs.camera((1.07, 1.13, 2.57), (3.6, 4.2, 0.5), 45.0), rs.camera((1.53, 2.1, 2.16), (3.8, 4.6, 0.6), 40.0), rs.camera((6.47, 6.03, 1.61), (x, y, 0.6), 45.0)]
    return _scene(bs, [0, 1, 2], cams, rs._tilted_map(), far=12.0, goals=g, cur_goal_idx=[0, 1, 2], reached=[0, 1, 0], goal_radius=float(np.float32(0.1)))


def static_scene():
    """render_scenes.heightfield_scene with three empty slots and one goal out of view: the flag-off image"""
    s = rs.heightfield_scene()
    s.update(obst_desc=rs._f32(np.zeros((1, 3, 8))), obst_state=rs._f32(np.zeros((1, 3, 4))), goals=rs._f32([[[-40.0, -40.0, 0.5]]]), cur_goal_idx=[0], reached=[0],
             goal_radius=float(np.float32(0.1)))
    return s


SCENES = dict(seesaw=seesaw_scene, bar_tyre=bar_tyre_scene, bar_tyre_61x35=lambda: bar_tyre_scene(61, 35), goals=goals_scene, static=static_scene)


@functools.lru_cache(maxsize=None)
def scene(name):
    return rs.attach(SCENES[name]())


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """(ids, depth, rgb, edge) of camera k, float64"""
    return rc.render(scene(name), k)
