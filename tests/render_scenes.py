"""Scenes shared by tests/test_render_cpu.py (the reference's own edge-pixel share) and tests/test_render.py (the kernel against the
reference).  Every number a scene holds is representable in fp32, so the kernel and the float64 reference start from the same inputs."""
import numpy as np

from tests import render_ref as rr

W, H = 64, 48
FAR_AWAY = 500.0


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def parked_rows():
    """19 body rows far behind every camera (the renderer always draws all 19 bodies: a scene of single primitives parks the others)"""
    rows = np.zeros((19, 13))
    rows[:, 0] = FAR_AWAY + 2.0 * np.arange(19); rows[:, 1] = FAR_AWAY; rows[:, 2] = 0.5; rows[:, 6] = 1.0
    return rows


def camera(eye, target, fov_deg=60.0):
    return np.array(list(eye) + list(target) + [np.radians(fov_deg)])


def project(cam, width, height, point):
    """pixel (i, j) whose square holds the world point, by the renderer's camera model"""
    o = cam[:3]; f = cam[3:6] - o; f = f / np.linalg.norm(f)
    r = np.cross(f, [0, 0, 1.0]); r = r / np.linalg.norm(r); u = np.cross(r, f)
    v = np.asarray(point, np.float64) - o
    tv = np.tan(0.5 * cam[6]); th = tv * width / height
    sx, sy = (v @ r) / (v @ f), (v @ u) / (v @ f)
    return int(np.floor((1 - sy / tv) / 2 * height)), int(np.floor((sx / th + 1) / 2 * width))


def analytic_scene(width=W, height=H):
    """one box (base), one sphere (Head_lower) and one capsule (FL_hip) per env at chosen poses over the plane; N = 3, K = 2: envs 0 and 2
    with different cameras, env 1 a whole robot standing in both cameras' view -- a decoy that must not appear"""
    bs = np.stack([parked_rows() for _ in range(3)])
    bs[1] = rr.standing_body_state(root=(0.0, 0.0, 0.32))
    for e, (shift, turn) in ((0, (0.0, 0.3)), (2, (0.15, -0.8))):
        bs[e, 0, :3] = (0.0 + shift, 0.0, 0.45); bs[e, 0, 3:7] = _quat((0.3, 0.2, 1.0), turn)              # box
        bs[e, 2, :3] = (0.1, 0.55 + shift, 0.30); bs[e, 2, 3:7] = _quat((1, 0, 0), 0.4)                    # sphere
        bs[e, 3, :3] = (-0.1, -0.6 - shift, 0.35); bs[e, 3, 3:7] = _quat((0.2, 1.0, 0.4), 0.9 + turn)      # capsule (the hip's, offset 0.08 in its frame)
    cams = np.stack([camera((-1.6, -1.1, 1.2), (0.0, 0.0, 0.3), 50.0), camera((1.33, 1.47, 0.93), (0.0, 0.0, 0.3), 60.0)])
    return dict(body_state=_f32(bs), env_ids=[0, 2], cameras=_f32(cams), width=width, height=height, far=20.0,
                light_dir=_f32((0.35, 0.25, 1.0)), flags=3, terrain=None)


def standing_scene():
    """a whole Go2 standing on the plane, seen by a follow camera at the reference's camera_pos_bias and from the other side"""
    bs = rr.standing_body_state(root=(0.3, -0.2, 0.33), yaw=0.4)[None]
    root = bs[0, 0, :3]
    cams = np.stack([camera(root + (-2.8, -1.8, 1.8), root, 30.0), camera(root + (1.5, 1.6, 0.7), root, 40.0)])
    return dict(body_state=_f32(bs), env_ids=[0, 0], cameras=_f32(cams), width=W, height=H, far=20.0, light_dir=_f32((0.35, 0.25, 1.0)),
                flags=3, terrain=None)


HS, VS, BORDER, ROWS, COLS = 0.25, 0.005, 2.0, 48, 48


def _tilted_map():
    i, j = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    m = (2 * i + j).astype(np.int16)                    # a plane: 0.04 up per metre of x, 0.02 per metre of y
    m[20:24, 18:22] += 100                              # one raised block of cells, 0.5 m
    return m


def tilted_height(x, y):
    return VS * (2 * (x + BORDER) / HS + (y + BORDER) / HS)


def _terrain(hm, cm=None):
    return dict(height_samples=hm, ceiling_samples=cm, horizontal_scale=float(np.float32(HS)), vertical_scale=float(np.float32(VS)), border_size=BORDER)


def heightfield_scene():
    """(a) a tilted plane as an int16 map with one raised block, a robot standing on it; two cameras"""
    x, y = 4.0, 4.6
    bs = rr.standing_body_state(root=(x, y, 0.34 + tilted_height(x, y)), yaw=-0.5)[None]
    cams = np.stack([camera((1.0, 1.0, 2.6), (3.6, 3.2, 0.5), 55.0), camera((6.5, 6.0, 1.6), (x, y, 0.6), 45.0)])
    return dict(body_state=_f32(bs), env_ids=[0, 0], cameras=_f32(cams), width=W, height=H, far=12.0, light_dir=_f32((0.35, 0.25, 1.0)),
                flags=3, terrain=_terrain(_tilted_map()))


def ceiling_scene():
    """(b) a flat ceiling at 1.5 m over rows 10..40 with a hole in it, seen from underneath: ceiling where it exists, sky through the hole"""
    hm = np.zeros((ROWS, COLS), np.int16)
    cm = np.full((ROWS, COLS), rr.NO_CEILING, np.int16)
    cm[10:41, 4:44] = 300
    cm[22:28, 14:22] = rr.NO_CEILING
    bs = rr.standing_body_state(root=(3.0, 2.0, 0.33))[None]
    cams = np.stack([camera((0.5, 2.2, 0.6), (4.5, 2.4, 1.5), 60.0)])
    return dict(body_state=_f32(bs), env_ids=[0], cameras=_f32(cams), width=W, height=H, far=12.0, light_dir=_f32((0.35, 0.25, 1.0)),
                flags=3, terrain=_terrain(hm, cm))


def border_scene():
    """(c) a camera near the map's edge looking outwards: rays leave the map within `far`.  The lookup clamps, so the edge's height
    continues: the reference (and cell_of's semantics) imply GROUND there, not sky"""
    hm = _tilted_map()
    bs = rr.standing_body_state(root=(8.6, 3.0, 0.34 + tilted_height(8.6, 3.0)))[None]
    cams = np.stack([camera((7.23, 2.57, 1.9), (10.5, 3.2, 0.4), 60.0)])
    return dict(body_state=_f32(bs), env_ids=[0], cameras=_f32(cams), width=W, height=H, far=12.0, light_dir=_f32((0.35, 0.25, 1.0)),
                flags=3, terrain=_terrain(hm))


SHADOW_SPHERE, SHADOW_LIGHT, SHADOW_RADIUS = (0.75, 0.25, 0.5), (1.0, 0.0, 1.0), 0.047
SHADOW_CENTRE = (0.25, 0.25, 0.0)                       # the sphere's centre moved along -light to z = 0: the middle of the checker square [0, 0.5)^2
SHADOW_NEIGHBOUR = (0.25, 0.25 + 2 * SHADOW_RADIUS, 0.0)


def shadow_scene(flags=3):
    """a sphere (Head_lower, r 0.047) 0.5 m above the plane under a light 45 degrees off the vertical"""
    bs = parked_rows()[None].copy()
    bs[0, 2, :3] = SHADOW_SPHERE
    cams = np.stack([camera((0.25, -1.0, 1.0), SHADOW_CENTRE, 20.0)])
    return dict(body_state=_f32(bs), env_ids=[0], cameras=_f32(cams), width=W, height=H, far=20.0, light_dir=_f32(SHADOW_LIGHT),
                flags=flags, terrain=None)


def attach(scene):
    """the table and palette of the built library (host calls: no device)"""
    from quadrupedal_agility_amd import render
    scene["table"], scene["palette"] = render.shape_table(), render.palette()
    return scene


def cpu_scenes():
    s = dict(analytic=analytic_scene(), analytic_61x35=analytic_scene(61, 35), standing=standing_scene(), heightfield=heightfield_scene(),
             ceiling=ceiling_scene(), border=border_scene(), shadow=shadow_scene())
    return {k: attach(v) for k, v in s.items()}
