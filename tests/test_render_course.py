"""The course mode of the frame renderer (include/qa_render_course.h, csrc/qa_render_course.hip) on the GPU against the float64 reference
tests/render_course_ref.py, by tests/test_render.py's rule: ids equal, colours within one level, edge pixels (at most 1 % per camera) excluded."""
import os
import types

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd import _capi
from tests import render_course_scenes as cs
from tests.test_render import GUARD, SENTINEL_F32, SENTINEL_I8, SENTINEL_U8
from tests.test_render_course_cpu import compare_camera

pytestmark = pytest.mark.gpu

# |depth_fp32 - depth_float64| / max(1, depth) off the edge pixels.  tests/test_render.py's bound is 4 x 1.211e-6.  The course scenes measure
# 1.076e-6 at most on the GPU (profiles/render_course_parity.json, written by tools/render_course_parity.py: the bar and tyre scene, camera
# 0), which is not larger, so that bound stands here; the ceiling for a measured value is 1e-4, the margin covers other poses.
DEPTH_REL_MEASURED = 1.211e-6
DEPTH_REL_TOL = 4 * DEPTH_REL_MEASURED
DEV = "cuda:0"


def gpu_render(scene, guard=False, course=True, **over):
    """the scene on the GPU: ids (K,H,W), depth, rgb as numpy; with `guard` inside sentinel-filled buffers that are returned too"""
    from quadrupedal_agility_amd.render import render_frames
    K, Hh, Ww = len(scene["env_ids"]), scene["height"], scene["width"]
    g = GUARD if guard else 0
    bufs = [torch.full((K * Hh * Ww * 3 + 2 * g,), SENTINEL_U8, dtype=torch.uint8, device=DEV), torch.full((K * Hh * Ww + 2 * g,), SENTINEL_F32, device=DEV),
            torch.full((K * Hh * Ww + 2 * g,), SENTINEL_I8, dtype=torch.int8, device=DEV)]
    rgb = bufs[0][g:g + K * Hh * Ww * 3].view(K, Hh, Ww, 3); depth = bufs[1][g:g + K * Hh * Ww].view(K, Hh, Ww); ids = bufs[2][g:g + K * Hh * Ww].view(K, Hh, Ww)
    t = scene["terrain"]
    kw = dict(height_samples=torch.from_numpy(np.ascontiguousarray(t["height_samples"])).to(DEV), border_size=t["border_size"],
              horizontal_scale=t["horizontal_scale"], vertical_scale=t["vertical_scale"])
    if t.get("ceiling_samples") is not None:
        kw["ceiling_samples"] = torch.from_numpy(np.ascontiguousarray(t["ceiling_samples"])).to(DEV)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)
    if course and scene.get("obst_desc") is not None:
        kw.update(obst_desc=f32(scene["obst_desc"]), obst_state=f32(scene["obst_state"]))
    if course and scene.get("goals") is not None:
        kw.update(goals=f32(scene["goals"]), cur_goal_idx=torch.tensor(scene["cur_goal_idx"], dtype=torch.long, device=DEV),
                  reached=torch.tensor(scene["reached"], dtype=torch.uint8, device=DEV), goal_radius=scene["goal_radius"])
    kw.update(over)
    render_frames(f32(scene["body_state"]), torch.tensor(scene["env_ids"], dtype=torch.int32, device=DEV), f32(scene["cameras"]), rgb, depth=depth, ids=ids,
                  far=scene["far"], light_dir=tuple(scene["light_dir"]), shadows=bool(scene["flags"] & 1), checker=bool(scene["flags"] & 2), **kw)
    torch.cuda.synchronize()
    out = ids.cpu().numpy().astype(np.int64), depth.cpu().numpy().astype(np.float64), rgb.cpu().numpy()
    return out + (tuple(b.cpu().numpy() for b in bufs),) if guard else out


def compare(name, got=None):
    scene = cs.scene(name)
    ids, depth, rgb = got if got is not None else gpu_render(scene)
    return max(compare_camera(name, k, ids[k], depth[k], rgb[k], DEPTH_REL_TOL) for k in range(len(scene["env_ids"])))


# ------------------------------------------------------------------ 1. the drawn surface
def test_seesaw_at_both_stops_and_between_top_and_side_face():
    ids, depth, rgb = gpu_render(cs.scene("seesaw"))
    compare("seesaw", (ids, depth, rgb))
    for k in (0, 2):                                                 # from above: the plank's top, its near long side, the ground
        assert {19, 21, 22} <= set(np.unique(ids[k]).tolist())
    for k in (1, 3):                                                 # from beside, below the high end: the long side face
        assert (ids[k] == 22).sum() > 500 and not (ids[k] == 21).any()
    # cameras 0 and 1 look at env 0, 2 at env 1 (the other stop), 3 at env 2: another env's tilt would be another image
    assert not np.array_equal(ids[0], ids[2])


def test_bar_raised_tyre_lowered_with_its_ceiling_and_an_empty_slot():
    ids, depth, rgb = gpu_render(cs.scene("bar_tyre"))
    compare("bar_tyre", (ids, depth, rgb))
    seen = set(np.unique(ids).tolist())
    assert {19, 20, 21, 22} <= seen


def test_partial_tiles_write_nothing_outside_the_image():
    ids, depth, rgb, bufs = gpu_render(cs.scene("bar_tyre_61x35"), guard=True)
    compare("bar_tyre_61x35", (ids, depth, rgb))
    for b, s in zip(bufs, (SENTINEL_U8, SENTINEL_F32, SENTINEL_I8)):
        assert (b[:GUARD] == s).all() and (b[-GUARD:] == s).all()
    assert (ids != SENTINEL_I8).all() and (depth != SENTINEL_F32).all()


# ------------------------------------------------------------------ 2. goals
def test_goals_in_front_behind_and_half_sunk_with_the_current_and_reached_colours():
    scene = cs.scene("goals")
    assert scene["goals"].shape[1] == 26
    ids, depth, rgb = gpu_render(scene)
    compare("goals", (ids, depth, rgb))
    assert {23, 24} <= set(np.unique(ids[0]).tolist()) and {23, 25} <= set(np.unique(ids[1]).tolist()) and {23, 24} <= set(np.unique(ids[2]).tolist())
    for ident, col in ((23, (255, 0, 0)), (24, (0, 0, 255)), (25, (0, 255, 0))):          # red / blue / green up to the shade
        px = rgb[ids == ident].astype(int)
        hue = np.array(col) > 0
        assert (px[:, ~hue] == 0).all() and (px[:, hue] > 60).all()


def test_static_equivalence_all_kinds_zero_and_a_goal_out_of_view():
    scene = cs.scene("static")
    on, off = gpu_render(scene), gpu_render(scene, course=False)
    compare("static", on)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[2], off[2])
    assert (np.abs(on[1] - off[1]) / np.maximum(1.0, off[1])).max() <= DEPTH_REL_TOL


# ------------------------------------------------------------------ 3. the engine's own tensors
def _course_env(steps=3):
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    env = lr.LeggedRobot(make_cfg(4, 3), sim_device=DEV)
    for _ in range(steps):
        env.step(torch.zeros(env.num_envs, 12, device=env.device))
    torch.cuda.synchronize()
    return env


def _seesaw_camera(env):
    d = env.sim.t["OBST_DESC"][0, 0].cpu().numpy().astype(np.float64)          # slot 0 is the see-saw
    ax = np.array([d[2], d[3]])                                                # along the plank = along the lane: 1.5 m in front of its end
    eye = (d[0] - (d[4] + 1.5) * ax[0], d[1] - (d[4] + 1.5) * ax[1], 1.3)
    return eye, (d[0], d[1], 0.2)


def test_engine_scene_recorder_shows_obstacles_and_goals_and_the_default_does_not():
    from quadrupedal_agility_amd.render import FrameRecorder
    env = _course_env()
    assert env.articulated
    eye, target = _seesaw_camera(env)
    kw = dict(env_ids=(0,), size=(96, 64), camera="fixed", eye=eye, target=target, with_ids=True)
    rec = FrameRecorder(env, "unused", articulated=True, goals=True, **kw)
    rec.render()
    torch.cuda.synchronize()
    seen = set(np.unique(rec.ids.cpu().numpy()).tolist())
    assert 21 in seen and (23 in seen or 24 in seen), seen
    plain = FrameRecorder(env, "unused", **kw)
    plain.render()
    torch.cuda.synchronize()
    assert set(np.unique(plain.ids.cpu().numpy()).tolist()) <= set(range(-1, 21))
    # the frame follows the joint: the tensors are read when the launch executes
    before = rec.ids.clone()
    env.obst_state[0, 0, 0] = -env.obst_state[0, 0, 0]
    rec.render()
    torch.cuda.synchronize()
    assert not torch.equal(before, rec.ids)


def test_two_renders_are_bit_identical_and_recording_is_read_only(tmp_path):
    from quadrupedal_agility_amd.render import FrameRecorder
    scene = cs.scene("seesaw")
    a, b = gpu_render(scene), gpu_render(scene)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    env = _course_env()
    bk = env.bk
    snap = lambda: ({k: v.clone() for k, v in env.sim.t.items()}, env.env_goals.clone(), bk.cur_goal_idx.clone(), bk.reached_goal_ids.clone())
    s0 = snap()
    rec = FrameRecorder(env, str(tmp_path), env_ids=(0, 3), size=(64, 48), every=1, articulated=True, goals=True)
    assert len(rec.capture(0)) == 2
    torch.cuda.synchronize()
    s1 = snap()
    for name in s0[0]:
        assert torch.equal(s0[0][name], s1[0][name]), name
    for x, y in zip(s0[1:], s1[1:]):
        assert torch.equal(x, y)
    assert sorted(os.listdir(tmp_path)) == ["env0", "env3"]


# ------------------------------------------------------------------ 4. argument errors
def test_course_argument_errors_return_qa_e_arg_and_touch_nothing():
    import ctypes as C
    from quadrupedal_agility_amd.render import QaRenderCourse, RENDER_COURSE
    lib = _capi.load_library()
    n, K, Hh, Ww = 3, 2, 8, 8
    body = torch.zeros(n, 19, 13, device=DEV); body[..., 6] = 1
    env_ids = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    cams = torch.tensor([[0, -2, 1, 0, 0, 0, 1.0]] * 2, device=DEV)
    rgb = torch.full((K, Hh, Ww, 3), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    depth = torch.full((K, Hh, Ww), SENTINEL_F32, device=DEV); ids = torch.full((K, Hh, Ww), SENTINEL_I8, dtype=torch.int8, device=DEV)
    hm = torch.zeros(4, 4, dtype=torch.int16, device=DEV)
    desc, state, goals = torch.zeros(n, 3, 8, device=DEV), torch.zeros(n, 3, 4, device=DEV), torch.zeros(n, 4, 3, device=DEV)

    def call(**over):
        cfg, co = _capi.QaRenderCfg(), QaRenderCourse()
        cfg.num_envs, cfg.num_cameras, cfg.width, cfg.height, cfg.far, cfg.flags = n, K, Ww, Hh, 10.0, 3 | RENDER_COURSE
        cfg.terrain_type, cfg.map_rows, cfg.map_cols, cfg.horizontal_scale, cfg.vertical_scale = 1, 4, 4, 0.25, 0.005
        cfg.light_dir[2] = 1.0
        io = co.io
        io.body_state, io.env_ids, io.cameras, io.rgb, io.depth, io.ids, io.height_samples = (x.data_ptr() for x in (body, env_ids, cams, rgb, depth, ids, hm))
        co.obst_desc, co.obst_state, co.goals, co.num_goals, co.goal_radius = desc.data_ptr(), state.data_ptr(), goals.data_ptr(), 4, 0.1
        for k, v in over.items():
            setattr(cfg if hasattr(cfg, k) else co, k, v)
        return lib.qa_render_frames(C.byref(cfg), C.byref(co), _capi.stream(rgb))
    cases = [dict(terrain_type=0), dict(obst_desc=None), dict(obst_state=None), dict(obst_desc=None, obst_state=None, goals=None), dict(num_goals=0),
             dict(num_goals=33), dict(goal_radius=0.0), dict(goal_radius=-1.0)]
    for over in cases:
        assert call(**over) == -1, over
        assert b"qa_render_frames" in lib.qa_last_error()
    assert b"clear the flag" in (call(obst_desc=None, obst_state=None, goals=None), lib.qa_last_error())[1]
    torch.cuda.synchronize()
    assert (rgb == SENTINEL_U8).all() and (depth == SENTINEL_F32).all() and (ids == SENTINEL_I8).all()
    assert call() == 0                                               # and the same call without an error renders
    torch.cuda.synchronize()
    assert (ids != SENTINEL_I8).all()


# ------------------------------------------------------------------ 5. play, end to end
def test_tsc_play_records_course_frames(tmp_path, monkeypatch):
    from quadrupedal_agility_amd.tsc.legged_gym.scripts.play import play
    from quadrupedal_agility_amd.tsc.legged_gym.scripts.train import train
    from quadrupedal_agility_amd.tsc.legged_gym.utils import task_registry as tr_mod
    from quadrupedal_agility_amd.tsc.legged_gym.utils.helpers import get_args
    from tests.test_render_cpu import _decode_png
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    train(get_args(["--task", "go2", "--device", "gpu", "--num_envs", "4", "--max_iterations", "1", "--exptid", "rec001-x"]))
    frames = tmp_path / "frames"
    play(get_args(["--task", "go2", "--device", "gpu", "--num_envs", "4", "--exptid", "rec001-x", "--resumeid", "rec001-x", "--record_frames", str(frames),
                   "--record_articulated", "--record_goals", "--frame_size", "64x48"]), num_steps=6, quiet=True)
    assert sorted(os.listdir(frames)) == ["0.png", "1.png", "2.png"]
    imgs = [_decode_png(open(frames / f"{i}.png", "rb").read()) for i in range(3)]
    assert all(im.shape == (48, 64, 3) for im in imgs)
