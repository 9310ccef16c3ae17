"""Frames of the robot over its ground, for looking at a policy: the Python side of include/qa_render.h.

The reference's play scripts open Isaac Gym's viewer and, with RECORD_FRAMES, write every second frame to
logs/<experiment>/exported/frames/<n>.png (bbc/legged_gym/scripts/play.py:60,75-84).  There is no viewer here; `FrameRecorder` is that
branch: one HIP launch (csrc/qa_render.hip) ray-casts the chosen envs' robots -- the primitives of csrc/qa_render_shapes.h posed by
RIGID_BODY_STATE -- over the plane or the height field, and `write_png` stores the images with the standard library alone.  Read-only on the
engine: nothing of this is constructed unless play is started with --record_frames.  Video assembly is the user's business
(e.g. `ffmpeg -framerate 25 -i %d.png out.mp4`)."""
import ctypes as C
import math
import os
import struct
import zlib

import torch

from . import _capi
from . import _cdecl

DEFAULT_LIGHT = (0.35, 0.25, 1.0)
DEFAULT_FAR = 30.0
# include/qa_render_course.h: constants and one struct, no entry point -- read from the headers directly, _capi's public names stay as they are
QaRenderCourse = _cdecl.struct("qa_render_course")
RENDER_COURSE, RENDER_MAX_GOALS = _cdecl.values("QA_RENDER_", "COURSE MAX_GOALS")
DEFAULT_GOAL_RADIUS = 0.1               # the reference viewer's goal spheres (tsc legged_robot.py _draw_goals)


def _check(t, name, dtype, shape, device=None):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"render_frames: {name} must be a contiguous {dtype} tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"render_frames: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"render_frames: {name} is on {t.device}, expected {device}")


def render_frames(body_state, env_ids, cameras, rgb, depth=None, ids=None, height_samples=None, ceiling_samples=None, border_size=0.0,
                  horizontal_scale=0.0, vertical_scale=0.0, far=DEFAULT_FAR, light_dir=DEFAULT_LIGHT, shadows=True, checker=True,
                  env_ids_host=None, api=None, obst_desc=None, obst_state=None, goals=None, cur_goal_idx=None, reached=None,
                  goal_radius=DEFAULT_GOAL_RADIUS):
    """qa_render_frames on the current stream of `rgb`'s device.  body_state (N,19,13) fp32 (the engine's live RIGID_BODY_STATE), env_ids (K)
    int32, cameras (K,7) fp32 [eye, target, vertical fov in radians], rgb (K,H,W,3) uint8; optional depth (K,H,W) fp32 and ids (K,H,W) int8.
    `height_samples` (rows, cols) int16 selects the height field (else the plane z = 0), `ceiling_samples` the same grid.  `env_ids_host`: a
    CPU copy of env_ids; with it an entry outside [0, N) is refused, without it the kernel clamps.
    The course mode (include/qa_render_course.h; height field only): `obst_desc` (N,3,8) / `obst_state` (N,3,4) fp32, the env's live OBST_DESC
    and OBST_STATE, draw see-saw, bar and tyre in their joint state; `goals` (N,G,3) fp32 draws spheres of `goal_radius`, `cur_goal_idx` (N)
    int64 and `reached` (N) uint8 colour the current one.  All are read when the launch executes."""
    dev = rgb.device if torch.is_tensor(rgb) else None
    if not torch.is_tensor(rgb) or rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError("render_frames: rgb must be a (K,H,W,3) uint8 tensor")
    K, H, W = int(rgb.shape[0]), int(rgb.shape[1]), int(rgb.shape[2])
    _check(rgb, "rgb", torch.uint8, (K, H, W, 3))
    if not torch.is_tensor(body_state) or body_state.dim() != 3:
        raise ValueError("render_frames: body_state must be a (N,19,13) float32 tensor")
    N = int(body_state.shape[0])
    _check(body_state, "body_state", torch.float32, (N, len(_capi.BODY_NAMES), 13), dev)
    _check(env_ids, "env_ids", torch.int32, (K,), dev)
    _check(cameras, "cameras", torch.float32, (K, 7), dev)
    if depth is not None:
        _check(depth, "depth", torch.float32, (K, H, W), dev)
    if ids is not None:
        _check(ids, "ids", torch.int8, (K, H, W), dev)
    cfg, io = _capi.QaRenderCfg(), _capi.QaRenderIo()
    cfg.num_envs, cfg.num_cameras, cfg.width, cfg.height = N, K, W, H
    if height_samples is not None:
        if not torch.is_tensor(height_samples) or height_samples.dim() != 2:
            raise ValueError("render_frames: height_samples must be a (rows, cols) int16 tensor")
        _check(height_samples, "height_samples", torch.int16, tuple(height_samples.shape), dev)
        cfg.terrain_type, cfg.map_rows, cfg.map_cols = 1, int(height_samples.shape[0]), int(height_samples.shape[1])
        cfg.border_size, cfg.horizontal_scale, cfg.vertical_scale = float(border_size), float(horizontal_scale), float(vertical_scale)
        io.height_samples = height_samples.data_ptr()
        if ceiling_samples is not None:
            _check(ceiling_samples, "ceiling_samples", torch.int16, tuple(height_samples.shape), dev)
            io.ceiling_samples = ceiling_samples.data_ptr()
    elif ceiling_samples is not None:
        raise ValueError("render_frames: ceiling_samples without height_samples")
    cfg.far = float(far)
    for i in range(3):
        cfg.light_dir[i] = float(light_dir[i])
    cfg.flags = (_capi.RENDER_SHADOWS if shadows else 0) | (_capi.RENDER_CHECKER if checker else 0)
    if env_ids_host is not None:
        _check(env_ids_host, "env_ids_host", torch.int32, (K,), torch.device("cpu"))
        io.env_ids_host = env_ids_host.data_ptr()
    io.body_state, io.env_ids, io.cameras, io.rgb = body_state.data_ptr(), env_ids.data_ptr(), cameras.data_ptr(), rgb.data_ptr()
    io.depth = depth.data_ptr() if depth is not None else None
    io.ids = ids.data_ptr() if ids is not None else None
    if all(v is None for v in (obst_desc, obst_state, goals, cur_goal_idx, reached)):
        (api or _capi.API).launch("render_frames", C.byref(cfg), C.byref(io), on=rgb)
        return rgb
    if height_samples is None:
        raise ValueError("render_frames: obstacles and goals are drawn on the height field: height_samples is required")
    if (obst_desc is None) != (obst_state is None):
        raise ValueError("render_frames: obst_desc and obst_state go together")
    if goals is None and (cur_goal_idx is not None or reached is not None):
        raise ValueError("render_frames: cur_goal_idx / reached without goals")
    course = QaRenderCourse()
    course.io = io
    if obst_desc is not None:
        _check(obst_desc, "obst_desc", torch.float32, (N, 3, 8), dev)
        _check(obst_state, "obst_state", torch.float32, (N, 3, 4), dev)
        course.obst_desc, course.obst_state = obst_desc.data_ptr(), obst_state.data_ptr()
    if goals is not None:
        if not torch.is_tensor(goals) or goals.dim() != 3 or not 1 <= int(goals.shape[1]) <= RENDER_MAX_GOALS:
            raise ValueError(f"render_frames: goals must be a (N,G,3) float32 tensor with 1 <= G <= {RENDER_MAX_GOALS}")
        _check(goals, "goals", torch.float32, (N, int(goals.shape[1]), 3), dev)
        if not float(goal_radius) > 0.0:
            raise ValueError(f"render_frames: goal_radius = {goal_radius}")
        course.goals, course.num_goals, course.goal_radius = goals.data_ptr(), int(goals.shape[1]), float(goal_radius)
        if cur_goal_idx is not None:
            _check(cur_goal_idx, "cur_goal_idx", torch.int64, (N,), dev)
            course.cur_goal_idx = cur_goal_idx.data_ptr()
        if reached is not None:
            _check(reached, "reached", torch.uint8, (N,), dev)
            course.reached = reached.data_ptr()
    cfg.flags |= RENDER_COURSE
    (api or _capi.API).launch("render_frames", C.byref(cfg), C.byref(course), on=rgb)
    return rgb


def shape_table(lib=None):
    """the primitive table the library was built with (csrc/qa_render_shapes.h): a list of dicts kind / body / cls / a / b / r"""
    lib = lib or _capi.load_library()
    n = lib.qa_render_shape_table(None, 0)
    buf = (C.c_float * (10 * n))()
    lib.qa_render_shape_table(buf, n)
    return [dict(kind=int(buf[10 * i]), body=int(buf[10 * i + 1]), cls=int(buf[10 * i + 2]), a=tuple(buf[10 * i + 3:10 * i + 6]),
                 b=tuple(buf[10 * i + 6:10 * i + 9]), r=float(buf[10 * i + 9])) for i in range(n)]


def palette(lib=None):
    """the renderer's colour per class (trunk, hip, thigh, calf, foot, ground, ceiling, sky), floats in [0, 1]"""
    lib = lib or _capi.load_library()
    buf = (C.c_float * 64)()
    n = lib.qa_render_palette(buf)
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, array):
    """An (H, W, 3) uint8 array (numpy, or anything with .shape and .tobytes() after a uint8 cast) as an 8-bit RGB PNG: filter type 0 on every
    scanline, one IDAT chunk, standard library only."""
    import numpy as np
    a = np.ascontiguousarray(array)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"write_png: expected an (H, W, 3) uint8 array, got {a.shape} {a.dtype}")
    h, w = int(a.shape[0]), int(a.shape[1])
    raw = np.zeros((h, 1 + 3 * w), np.uint8)            # a filter byte of 0 (None) in front of every scanline
    raw[:, 1:] = a.reshape(h, 3 * w)
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b"")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


class FrameRecorder:
    """RECORD_FRAMES of the reference's play loop on an env of either tree (anything with `.sim`, a QaSim whose engine exports body state).

    `camera="follow"`: eye = root position + `offset`, target = the root, per recorded env (the reference's MOVE_CAMERA branch with its
    camera_pos_bias); `camera="fixed"`: `eye` / `target` as given, one pair for all envs or one per env.  The camera rows are computed from
    ROOT_STATES with torch ops on the device: `render()` does not synchronise.  `capture(i)` renders when i % every == 0, copies the images
    to the host and writes <out_dir>/<img_idx>.png (one env) or <out_dir>/env<id>/<img_idx>.png (several)."""

    def __init__(self, env, out_dir, env_ids=(0,), size=(640, 360), every=2, camera="follow", offset=(-2.8, -1.8, 1.8), fov_deg=60.0,
                 eye=None, target=None, far=DEFAULT_FAR, light_dir=DEFAULT_LIGHT, shadows=True, checker=True, with_ids=False,
                 articulated=False, goals=False, goal_radius=DEFAULT_GOAL_RADIUS):
        sim = env.sim
        q = sim.cfg
        if not int(q.export_body_state):
            raise RuntimeError("FrameRecorder needs the engine's body poses: build the env with sim.qa.export_body_state = 1 "
                               "(play.py --record_frames sets it); this engine was created without RIGID_BODY_STATE")
        self.env_ids_list = [int(e) for e in env_ids]
        n = int(q.num_envs)
        if not self.env_ids_list or any(e < 0 or e >= n for e in self.env_ids_list):
            raise ValueError(f"FrameRecorder: env_ids {self.env_ids_list} must name at least one env of [0, {n})")
        if camera not in ("follow", "fixed"):
            raise ValueError("FrameRecorder: camera is 'follow' or 'fixed'")
        if camera == "fixed" and (eye is None or target is None):
            raise ValueError("FrameRecorder: camera='fixed' takes eye= and target=")
        self.width, self.height = int(size[0]), int(size[1])
        self.every, self.out_dir, self.camera = max(1, int(every)), out_dir, camera
        dev = sim.device
        k = len(self.env_ids_list)
        self.body_state, self.root_states = sim.t["RIGID_BODY_STATE"], sim.t["ROOT_STATES"]
        self._ids_host = torch.tensor(self.env_ids_list, dtype=torch.int32)
        self.env_ids = self._ids_host.to(dev)
        self._index = self.env_ids.long()
        self.offset = torch.tensor([float(v) for v in offset], dtype=torch.float32, device=dev)
        self.cameras = torch.zeros(k, 7, dtype=torch.float32, device=dev)
        self.cameras[:, 6] = math.radians(float(fov_deg))
        if camera == "fixed":
            self.cameras[:, 0:3] = torch.as_tensor(eye, dtype=torch.float32, device=dev).reshape(-1, 3)
            self.cameras[:, 3:6] = torch.as_tensor(target, dtype=torch.float32, device=dev).reshape(-1, 3)
        self.rgb = torch.zeros(k, self.height, self.width, 3, dtype=torch.uint8, device=dev)
        self.ids = torch.zeros(k, self.height, self.width, dtype=torch.int8, device=dev) if with_ids else None
        self._terrain = {}
        if int(q.terrain_type) == 1:
            self._terrain = dict(height_samples=sim.t["HEIGHT_SAMPLES"], border_size=float(q.hf_border), horizontal_scale=float(q.hf_hscale),
                                 vertical_scale=float(q.hf_vscale), ceiling_samples=sim.t["CEILING_SAMPLES"] if int(q.hf_ceiling) else None)
        self._opts = dict(far=far, light_dir=light_dir, shadows=shadows, checker=checker)
        # the course as the physics has it and the goals (include/qa_render_course.h): the env's own live tensors, nothing is copied
        if articulated:
            if not getattr(env, "articulated", False):
                raise ValueError("FrameRecorder: articulated=True needs an env whose see-saw, bar and tyre are articulated bodies "
                                 "(the task-level tree with articulated_obstacles): this env keeps the static maps")
            self._opts.update(obst_desc=sim.t["OBST_DESC"], obst_state=env.obst_state)
        if goals:
            bk = getattr(env, "bk", None)
            if not hasattr(env, "env_goals") or bk is None:
                raise ValueError("FrameRecorder: goals=True needs an env with goals (the task-level tree's env_goals and goal bookkeeping)")
            self._opts.update(goals=env.env_goals, cur_goal_idx=bk.cur_goal_idx, reached=bk.reached_goal_ids, goal_radius=goal_radius)
        self._api = sim.api
        self.img_idx = 0

    def render(self):
        """the (K,H,W,3) uint8 device tensor of the current state (the recorder's own buffer: the next render overwrites it)"""
        if self.camera == "follow":
            pos = self.root_states[self._index, 0:3]
            self.cameras[:, 0:3] = pos + self.offset
            self.cameras[:, 3:6] = pos
        return render_frames(self.body_state, self.env_ids, self.cameras, self.rgb, ids=self.ids, env_ids_host=self._ids_host, api=self._api,
                             **self._terrain, **self._opts)

    def path(self, k, img_idx):
        if len(self.env_ids_list) == 1:
            return os.path.join(self.out_dir, f"{img_idx}.png")
        return os.path.join(self.out_dir, f"env{self.env_ids_list[k]}", f"{img_idx}.png")

    def capture(self, i):
        """step i of the play loop: every `every`-th step becomes one PNG per recorded env; returns the paths written"""
        if i % self.every:
            return []
        frames = self.render().cpu().numpy()
        paths = [write_png(self.path(k, self.img_idx), frames[k]) for k in range(frames.shape[0])]
        self.img_idx += 1
        return paths


def add_record_args(parser):
    """the play scripts' recording flags (both trees' helpers.get_args)"""
    parser.add_argument("--record_frames", nargs="?", const="", default=None, metavar="DIR",
                        help="write every --record_every-th frame of the play loop as a PNG into DIR (default logs/<experiment_name>/exported/frames)")
    parser.add_argument("--record_envs", type=str, default="0", help="comma-separated env ids to record, e.g. 0,3")
    parser.add_argument("--record_every", type=int, default=2, help="record every N-th step (the reference records every second one)")
    parser.add_argument("--frame_size", type=str, default="640x360", metavar="WxH")
    parser.add_argument("--record_offset", type=str, default=None, metavar="X,Y,Z",
                        help="the follow camera's eye relative to the robot's root, world axes (default: the reference's camera_pos_bias -2.8,-1.8,1.8; "
                             "on the obstacle course 0,-1.2,2.6, inside the lane's 2 m walls)")
    parser.add_argument("--record_articulated", action="store_true", default=False,
                        help="draw see-saw, bar and tyre in their joint state, as the physics has them (the task-level tree with articulated obstacles)")
    parser.add_argument("--record_goals", action="store_true", default=False, help="draw the env's goals as spheres: red, the current one blue, green once reached")


COURSE_OFFSET = (0.0, -1.2, 2.6)       # the course's lanes run along +y between 2 m walls: the reference's bias would put the eye behind one


def record_settings(args, experiment_name, default_offset=None):
    """None without --record_frames; else the FrameRecorder arguments the flags ask for (`offset` only when the flags or the caller name one)"""
    rec = getattr(args, "record_frames", None)
    if rec is None:
        return None
    out_dir = rec or os.path.join("logs", str(experiment_name), "exported", "frames")
    try:
        w, h = (int(v) for v in str(getattr(args, "frame_size", "640x360")).lower().split("x"))
        env_ids = tuple(int(v) for v in str(getattr(args, "record_envs", "0")).split(",") if v.strip() != "")
        off = getattr(args, "record_offset", None)
        offset = tuple(float(v) for v in off.split(",")) if off else default_offset
        if offset is not None and len(offset) != 3:
            raise ValueError
    except ValueError:
        raise ValueError("--frame_size takes WxH (e.g. 640x360), --record_envs comma-separated env ids (e.g. 0,3), --record_offset X,Y,Z")
    out = dict(out_dir=out_dir, env_ids=env_ids, size=(w, h), every=int(getattr(args, "record_every", 2)))
    if offset is not None:
        out["offset"] = offset
    for flag, key in (("record_articulated", "articulated"), ("record_goals", "goals")):
        if getattr(args, flag, False):
            out[key] = True
    return out
