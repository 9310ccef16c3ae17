"""Scenes shared by tests/test_depth_obstacles_cpu.py and tests/test_depth_obstacles.py: the analytic see-saw and bar scenes (closed-form
depth per pixel), and cameras placed in front of the see-saws, bars and tyres of a generated course."""
import functools

import numpy as np
import torch

from quadrupedal_agility_amd import _capi
from tests import depth_obstacles_ref as ref
from tests.test_tsc_depth import CAM, FAR, H, NEAR, TAN_H, TAN_V, W

MAX_TILT = float(np.float32(0.16744808))            # QA_SEESAW_MAX_TILT
SEESAW_TILTS = (MAX_TILT, -MAX_TILT, 0.05)
SEESAW_YAWS = (0.0, 0.6)
STEP_XY = 0.5 * 0.05                                 # a march step moves at most hs / 2 in the plane
ROOT_Z = 0.6                                         # the camera (0.698 m) looks down on the plank's high end (0.51 m)


def rays_yaw0(wc, hc, crop_left, crop_top):
    """camera-frame rays (forward component 1: t is the planar depth) of the cropped pixels for a level trunk at yaw 0, pitch 0"""
    r = np.arange(hc)[:, None] + crop_top; c = np.arange(wc)[None, :] + crop_left
    sx = ((c + 0.5) / W * 2 - 1) * TAN_H; sy = ((r + 0.5) / H * 2 - 1) * TAN_V
    return np.broadcast_arrays(1.0 + 0 * sx * sy, -sx + 0 * sy, -sy + 0 * sx)


def flat_scene(z=ROOT_Z):
    """scene() of tests/test_tsc_depth.py with the trunk at height z: root (1,13), pitch (1), a zero 200 x 200 map"""
    from tests.test_tsc_depth import scene
    root, pitch, hmap, ep, _ = scene(z=z)
    return root, pitch, hmap, ep


def camera_origin(root):
    return root[0, :3].double().numpy() + CAM


def seesaw_record(root, yaw, q):
    """one see-saw (plank 3.0 x 0.6 m, pivot 0.26 m up) whose origin lies 1.5 m ahead of the camera, turned by `yaw`, tilted by q"""
    o = camera_origin(root)
    desc = np.zeros((1, 3, 8), np.float32); state = np.zeros((1, 3, 4), np.float32)
    desc[0, 0] = [o[0] + 1.5, o[1], np.cos(yaw), np.sin(yaw), 1.5, 0.3, 0.26, _capi.OBST_SEESAW]
    state[0, 0, 0] = q
    return desc, state


def seesaw_analytic(root, desc, state, wc, hc, crop_left=10, crop_top=1):
    """depth of the plank's top plane per pixel, the pixels that see it (`plank`) and the ones of them whose hit lies more than one march
    step from a footprint edge and from the line where the plank meets the ground (`keep`)"""
    o = camera_origin(root)
    d = [float(v) for v in desc[0, 0]]; q = float(state[0, 0, 0]); tq = np.tan(q)
    dx, dy, dz = rays_yaw0(wc, hc, crop_left, crop_top)
    c, s, h0 = d[2], d[3], d[6]
    lx_o = c * (o[0] - d[0]) + s * (o[1] - d[1]); ly_o = c * (o[1] - d[1]) - s * (o[0] - d[0])
    dl, dm = c * dx + s * dy, c * dy - s * dx
    f0 = o[2] - (h0 - lx_o * tq)                                      # height of the camera over the plane's extension
    den = dl * tq + dz
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den < 0, -f0 / den, np.inf)
    lx, ly, z = lx_o + t * dl, ly_o + t * dm, o[2] + t * dz
    with np.errstate(invalid="ignore"):
        plank = (f0 > 0) & (t > NEAR) & (t < FAR) & (np.abs(lx) <= d[4]) & (np.abs(ly) <= d[5]) & (z > 0)
        edge = np.minimum(d[4] - np.abs(lx), d[5] - np.abs(ly))
        ground_line = np.abs(lx - h0 / tq)                             # where h0 - lx tan q = 0
        keep = plank & (edge > STEP_XY) & (ground_line > STEP_XY)
    return t, plank, keep


BOX_H, BOX_X, BOX_HALF = 60, 3.5, (0.2, 0.5)                          # a 0.30 m box, its centre, the half sizes of its top face


def bar_scene(q):
    """a box drawn in the map 1.2 m ahead of the camera, and a bar record whose footprint covers it and the one-cell ramps around it"""
    root, pitch, hmap, ep = flat_scene()
    xs = np.arange(200) * 0.05 - 1.0
    ix = np.nonzero(np.abs(xs - BOX_X) <= BOX_HALF[0] + 1e-9)[0]; iy = np.nonzero(np.abs(xs - 4.0) <= BOX_HALF[1] + 1e-9)[0]
    hmap[ix[0]:ix[-1] + 1, iy[0]:iy[-1] + 1] = BOX_H
    desc = np.zeros((1, 3, 8), np.float32); state = np.zeros((1, 3, 4), np.float32)
    desc[0, 1] = [BOX_X, 4.0, 1.0, 0.0, 0.3, 0.6, 0.0, _capi.OBST_BAR]
    state[0, 1, 0] = q
    return root, pitch, hmap, ep, desc, state


def bar_analytic(root, state, wc, hc, crop_left=10, crop_top=1):
    o = camera_origin(root)
    top = BOX_H * 0.005 + float(state[0, 1, 0])
    dx, dy, dz = rays_yaw0(wc, hc, crop_left, crop_top)
    with np.errstate(divide="ignore"):
        t = np.where(dz < 0, (o[2] - top) / -dz, np.inf)
    x, y = o[0] + t * dx, o[1] + t * dy
    with np.errstate(invalid="ignore"):
        keep = (t > NEAR) & (t < FAR) & (np.abs(x - BOX_X) < BOX_HALF[0] - STEP_XY) & (np.abs(y - 4.0) < BOX_HALF[1] - STEP_XY)
    return t, keep


def norm(t):
    return (np.clip(t, NEAR, FAR) - NEAR) / (FAR - NEAR) - 0.5


# ------------------------------------------------------------------ a generated course
KINDS = (("seesaw", 0, _capi.OBST_SEESAW, 1.5, 0.3, 0.26), ("bar_jump", 1, _capi.OBST_BAR, 0.1, 0.6, 0.0), ("tire_jump", 2, _capi.OBST_TYRE, 0.1, 0.4, 0.0))


def course_descriptors(ob, n):
    """QA_T_OBST_DESC as LeggedRobot._init_articulated_obstacles builds it"""
    desc = np.zeros((n, 3, 8), np.float32)
    for name, slot, kind, hx, hy, h0 in KINDS:
        t = ob.obst_types.index(name)
        for i in range(n):
            j = int(np.nonzero(ob.obstacle_types[i] == t)[0][0])
            yaw = ob.obstacle_yaws[i, j]
            desc[i, slot] = [ob.obstacle_origins[i, j, 0], ob.obstacle_origins[i, j, 1], np.cos(yaw), np.sin(yaw), hx, hy, h0, kind]
    return desc


@functools.lru_cache(maxsize=None)
def course(n=16, seed=1):
    """Obstacle(LeggedRobotCfg.obstacle(), n, seed): env i's robot stands 1.0 .. 2.0 m from the origin of its see-saw (i % 3 == 0; 1.6 .. 2.0 m,
    beyond the plank's low end), bar (1) or tyre (2), facing it within +-0.15 rad, trunk 0.25 .. 0.45 m over the rendered floor.  Joint positions: uniform in
    +-QA_SEESAW_MAX_TILT (see-saws) and +-0.05 m (bars, tyres), the first envs of each kind at the extremes."""
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    from quadrupedal_agility_amd.tsc.legged_gym.utils.obstacle import Obstacle
    ob = Obstacle(LeggedRobotCfg.obstacle(), n, seed=seed)
    rng = np.random.default_rng(seed)
    desc = course_descriptors(ob, n)
    state = np.zeros((n, 3, 4), np.float32)
    state[:, 0, 0] = rng.uniform(-MAX_TILT, MAX_TILT, n); state[:, 1:, 0] = rng.uniform(-0.05, 0.05, (n, 2))
    state[0, 0, 0], state[3, 0, 0] = MAX_TILT, -MAX_TILT
    state[1, 1, 0], state[4, 1, 0], state[2, 2, 0], state[5, 2, 0] = 0.05, -0.05, 0.05, -0.05
    state[:, :, 1] = rng.uniform(-1, 1, (n, 3)); state[:, 0, 3] = rng.uniform(1, 10, n)         # q_dot and damping: never read by the render
    hmap, cmap = np.ascontiguousarray(ob.height_field_raw), np.ascontiguousarray(ob.ceiling_raw)
    root = np.zeros((n, 13), np.float32)
    for i in range(n):
        d = desc[i, i % 3]
        psi = np.arctan2(d[3], d[2])
        r, off = rng.uniform(1.6, 2.0) if i % 3 == 0 else rng.uniform(1.0, 2.0), rng.uniform(-0.3, 0.3)     # (see-saws: in front of the plank's end)
        side = 1.0 if (i % 3 == 0 and state[i, 0, 0] > 0) else -1.0                      # a see-saw is met at its low end: lx > 0 when q > 0
        pos = d[:2] + side * r * np.array([np.cos(psi + off), np.sin(psi + off)])
        yaw = np.arctan2(d[1] - pos[1], d[0] - pos[0]) + rng.uniform(-0.15, 0.15)
        rec = ref.records(desc[i], state[i])
        fl, _ = ref.tri_height(hmap, pos[0], pos[1], 5.0, 0.05, 0.005)
        fl = ref.surface(rec, pos[0], pos[1], fl, fl)[0]
        root[i, :3] = [pos[0], pos[1], fl + rng.uniform(0.25, 0.45)]
        rpy = [rng.uniform(-0.1, 0.1), rng.uniform(-0.15, 0.15), yaw]
        cr, sr, cp, sp, cy, sy = (f(a / 2) for a in rpy for f in (np.cos, np.sin))
        root[i, 3:7] = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]
    pitch = np.radians(rng.uniform(-5, 5, n)).astype(np.float32)
    ep = rng.integers(0, 4, n)
    ep[0], ep[1] = 0, 3                                                # both ring modes, whatever the draw
    return dict(ob=ob, hmap=torch.from_numpy(hmap), cmap=torch.from_numpy(cmap), root=torch.from_numpy(root), pitch=torch.from_numpy(pitch),
                ep=torch.from_numpy(ep).long(), desc=torch.from_numpy(desc), state=torch.from_numpy(state))
