"""The frame renderer (include/qa_render.h, csrc/qa_render.hip, quadrupedal_agility_amd/render.py) on the GPU against the float64 reference
tests/render_ref.py, off the reference's edge pixels (at most 1 % of a scene's pixels may be excluded)."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd import _capi
from tests import render_ref as rr
from tests import render_scenes as rs

pytestmark = pytest.mark.gpu

# |depth_fp32 - depth_float64| / max(1, depth) off the edge pixels: 4 x the largest value measured on the GPU over the scenes of cases 1-3
# (profiles/render_parity.json, written by tools/render_parity.py: 1.211e-6, on one of the engine-posed robots).  The margin covers other
# poses than the ones measured; the ceiling for the measured value itself is 1e-4.
DEPTH_REL_MEASURED = 1.211e-6
DEPTH_REL_TOL = 4 * DEPTH_REL_MEASURED
EDGE_CAP = 0.01
SENTINEL_U8, SENTINEL_F32, SENTINEL_I8 = 0xA7, -77.0, 99
GUARD = 7


def gpu_render(scene, guard=False):
    """the scene on the GPU: ids (K,H,W), depth, rgb as numpy; with `guard`, the outputs sit inside sentinel-filled buffers that are returned too"""
    dev = "cuda:0"
    K, Hh, Ww = len(scene["env_ids"]), scene["height"], scene["width"]
    g = GUARD if guard else 0
    bufs = [torch.full((K * Hh * Ww * 3 + 2 * g,), SENTINEL_U8, dtype=torch.uint8, device=dev), torch.full((K * Hh * Ww + 2 * g,), SENTINEL_F32, device=dev),
            torch.full((K * Hh * Ww + 2 * g,), SENTINEL_I8, dtype=torch.int8, device=dev)]
    rgb = bufs[0][g:g + K * Hh * Ww * 3].view(K, Hh, Ww, 3); depth = bufs[1][g:g + K * Hh * Ww].view(K, Hh, Ww); ids = bufs[2][g:g + K * Hh * Ww].view(K, Hh, Ww)
    from quadrupedal_agility_amd.render import render_frames
    t = scene.get("terrain") or {}
    kw = {}
    if t:
        kw = dict(height_samples=torch.from_numpy(np.ascontiguousarray(t["height_samples"])).to(dev), border_size=t["border_size"],
                  horizontal_scale=t["horizontal_scale"], vertical_scale=t["vertical_scale"])
        if t.get("ceiling_samples") is not None:
            kw["ceiling_samples"] = torch.from_numpy(np.ascontiguousarray(t["ceiling_samples"])).to(dev)
    body = scene.get("body_state_device")
    if body is None:
        body = torch.from_numpy(scene["body_state"].astype(np.float32)).to(dev)
    render_frames(body, torch.tensor(scene["env_ids"], dtype=torch.int32, device=dev), torch.from_numpy(scene["cameras"].astype(np.float32)).to(dev),
                  rgb, depth=depth, ids=ids, far=scene["far"], light_dir=tuple(scene["light_dir"]), shadows=bool(scene["flags"] & 1),
                  checker=bool(scene["flags"] & 2), **kw)
    torch.cuda.synchronize()
    out = ids.cpu().numpy().astype(np.int64), depth.cpu().numpy().astype(np.float64), rgb.cpu().numpy()
    return out + (tuple(b.cpu().numpy() for b in bufs),) if guard else out


def compare(scene, name, got=None):
    """kernel against reference, camera by camera; returns the largest relative depth error off the edges"""
    ids, depth, rgb = got if got is not None else gpu_render(scene)
    worst = 0.0
    for k in range(len(scene["env_ids"])):
        rid, rdepth, rrgb, edge = rr.render(scene, k)
        assert edge.mean() <= EDGE_CAP, (name, k, edge.mean())
        ok = ~edge
        bad = ok & (ids[k] != rid)
        assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:5].tolist(), ids[k][bad][:5], rid[bad][:5])
        rel = np.abs(depth[k] - rdepth) / np.maximum(1.0, rdepth)
        err = float(rel[ok].max())
        diff = np.abs(rgb[k].astype(np.int64) - rrgb.astype(np.int64)).max(axis=-1)
        print(f"{name} camera {k}: edge share {edge.mean():.4%}, depth rel err {err:.3e}, rgb pixels off by one level {float((diff[ok] > 0).mean()):.4%}, "
              f"ids {sorted(set(rid.ravel().tolist()))}")
        worst = max(worst, err)
        assert err <= DEPTH_REL_TOL, (name, k, err)
        assert diff[ok].max() <= 1, (name, k, int(diff[ok].max()), np.argwhere(ok & (diff > 1))[:5].tolist())
    return worst


@functools.lru_cache(maxsize=None)
def _scene(name, *args):
    return rs.attach(getattr(rs, name)(*args))


# ------------------------------------------------------------------ 1. analytic scenes
def test_single_primitives_over_the_plane_and_the_decoy_env_stays_out():
    scene = _scene("analytic_scene")
    ids, depth, rgb = gpu_render(scene)
    compare(scene, "analytic", (ids, depth, rgb))
    # env 0 shows its box, sphere and capsule (bodies 0, 2, 3) and nothing of env 1's whole robot standing in view
    assert set(np.unique(ids[0]).tolist()) == {-1, 0, 2, 3, 19} and set(np.unique(ids[1]).tolist()) <= {-1, 0, 2, 3, 19}
    assert not np.array_equal(rgb[0], rgb[1])


def test_partial_tiles_write_nothing_outside_the_image():
    scene = _scene("analytic_scene", 61, 35)
    ids, depth, rgb, bufs = gpu_render(scene, guard=True)
    compare(scene, "analytic 61x35", (ids, depth, rgb))
    for b, s in zip(bufs, (SENTINEL_U8, SENTINEL_F32, SENTINEL_I8)):
        assert (b[:GUARD] == s).all() and (b[-GUARD:] == s).all()
    assert (ids != SENTINEL_I8).all() and (depth != SENTINEL_F32).all()


# ------------------------------------------------------------------ 2. the robot as the engine poses it
def engine_scene():
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    n = 67
    sim = QaSim(go2_cfg(n, seed=4, export_body_state=1), "cuda:0")
    sim.reset_all()
    gen = torch.Generator().manual_seed(0)
    for _ in range(5):
        sim.step(torch.randn(n, 12, generator=gen).cuda())
    torch.cuda.synchronize()
    body = sim.t["RIGID_BODY_STATE"].clone()
    root = sim.t["ROOT_STATES"][:, :3].cpu().numpy().astype(np.float64)
    envs = [0, 33, 66, 0, 33, 66]
    # three follow cameras at the reference's camera_pos_bias and, so that the far side's legs are seen too, three from the other side
    cams = np.stack([rs.camera(root[e] + off, root[e], 14.0) for off, es in (((-2.8, -1.8, 1.8), envs[:3]), ((2.8, 1.8, 0.5), envs[3:])) for e in es])
    scene = dict(body_state=body.cpu().numpy().astype(np.float64), body_state_device=body, env_ids=envs, cameras=rs._f32(cams), width=rs.W, height=rs.H,
                 far=20.0, light_dir=rs._f32((0.35, 0.25, 1.0)), flags=3, terrain=None)
    return rs.attach(scene)


def test_engine_posed_robot_matches_the_reference_and_shows_every_body():
    scene = engine_scene()
    ids, depth, rgb = gpu_render(scene)
    compare(scene, "engine", (ids, depth, rgb))
    assert set(range(19)) <= set(np.unique(ids).tolist()), sorted(set(range(19)) - set(np.unique(ids).tolist()))


# ------------------------------------------------------------------ 3. height field
def test_tilted_plane_and_raised_block_against_the_exact_surface():
    scene = _scene("heightfield_scene")
    ids, depth, rgb = gpu_render(scene)
    compare(scene, "heightfield", (ids, depth, rgb))
    # the tilted plane is one plane: where the ground is hit away from the block, the depth is the closed-form ray / plane distance
    o, d = rr.camera_rays(scene["cameras"][0], rs.W, rs.H)
    nrm = np.array([-0.04, -0.02, 1.0]); p0 = np.array([0.0, 0.0, rs.tilted_height(0.0, 0.0)])
    tp = ((p0 - o) @ nrm) / (d @ nrm)
    hit = o + tp[:, None] * d
    # ground reached before the block's first sloped cell (x = 2.75): nothing can stand between the camera at x = 1 and such a point
    away = (ids[0].ravel() == 19) & (tp > 0) & (hit[:, 0] < 2.7)
    assert away.sum() > 100
    assert (np.abs(depth[0].ravel()[away] - tp[away]) / np.maximum(1.0, tp[away])).max() <= DEPTH_REL_TOL


def test_ceiling_where_it_exists_and_sky_through_the_hole():
    scene = _scene("ceiling_scene")
    ids, depth, rgb = gpu_render(scene)
    compare(scene, "ceiling", (ids, depth, rgb))
    assert (ids == 20).sum() > 200 and (ids == 19).sum() > 200
    # a ray that crosses z = 1.5 inside the hole's cells sees the sky; the hole's triangles need all three corners, so stay one cell inside
    o, d = rr.camera_rays(scene["cameras"][0], rs.W, rs.H)
    tc = (1.5 - o[2]) / np.where(d[:, 2] > 0, d[:, 2], np.nan)
    x, y = o[0] + tc * d[:, 0], o[1] + tc * d[:, 1]
    in_hole = (x > 23 * rs.HS - rs.BORDER) & (x < 26 * rs.HS - rs.BORDER) & (y > 15 * rs.HS - rs.BORDER) & (y < 20 * rs.HS - rs.BORDER)
    assert in_hole.sum() > 10 and (ids[0].ravel()[in_hole] == -1).all()


def test_rays_leaving_the_map_see_the_clamped_border():
    scene = _scene("border_scene")
    ids, depth, rgb = gpu_render(scene)
    compare(scene, "border", (ids, depth, rgb))
    o, d = rr.camera_rays(scene["cameras"][0], rs.W, rs.H)
    hx = o[0] + depth[0].ravel() * d[:, 0]
    outside = (ids[0].ravel() == 19) & (hx > (rs.ROWS - 1) * rs.HS - rs.BORDER + 0.1)
    assert outside.sum() > 100                                  # ground beyond the map's last sample: the edge's height continues


# ------------------------------------------------------------------ 4. shadow
def test_shadow_darkens_the_ground_under_the_sphere():
    lit = _scene("shadow_scene", 3)
    cam = lit["cameras"][0]
    ci, cj = rs.project(cam, rs.W, rs.H, rs.SHADOW_CENTRE)
    ni, nj = rs.project(cam, rs.W, rs.H, rs.SHADOW_NEIGHBOUR)
    ids, depth, rgb = gpu_render(lit)
    assert ids[0, ci, cj] == 19 and ids[0, ni, nj] == 19
    assert (rgb[0, ci, cj].astype(int) < rgb[0, ni, nj].astype(int)).all()
    _, _, rgb_off = gpu_render(_scene("shadow_scene", 2))
    assert np.array_equal(rgb_off[0, ci, cj], rgb_off[0, ni, nj]) and np.array_equal(rgb_off[0, ni, nj], rgb[0, ni, nj])
    compare(lit, "shadow", (ids, depth, rgb))


# ------------------------------------------------------------------ 5. read-only and deterministic
def test_two_renders_of_one_state_are_bit_identical():
    scene = _scene("heightfield_scene")
    a, b = gpu_render(scene), gpu_render(scene)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_recording_leaves_every_arena_tensor_bit_identical(tmp_path):
    from quadrupedal_agility_amd.render import FrameRecorder
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    n = 64
    arenas = []
    for record in (False, True):
        sim = QaSim(go2_cfg(n, seed=7, export_body_state=1), "cuda:0")
        sim.reset_all()
        rec = FrameRecorder(types.SimpleNamespace(sim=sim), str(tmp_path), env_ids=(0, 63), size=(64, 48), every=1) if record else None
        gen = torch.Generator().manual_seed(1)
        for i in range(10):
            sim.step(torch.randn(n, 12, generator=gen).cuda())
            if rec is not None:
                assert len(rec.capture(i)) == 2
        torch.cuda.synchronize()
        arenas.append({k: v.clone() for k, v in sim.t.items()})
    assert len(os.listdir(tmp_path / "env0")) == 10 and len(os.listdir(tmp_path / "env63")) == 10
    for name in _capi.TENSORS:
        if name != "EPISODE_STATS":                 # float atomicAdd order: differs between two runs of one build as well
            assert torch.equal(arenas[0][name], arenas[1][name]), name


def test_recorder_refuses_an_engine_without_body_state():
    from quadrupedal_agility_amd.render import FrameRecorder
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    sim = QaSim(go2_cfg(8, seed=1), "cuda:0")
    with pytest.raises(RuntimeError, match="export_body_state"):
        FrameRecorder(types.SimpleNamespace(sim=sim), "unused")


# ------------------------------------------------------------------ 6. play, end to end
def test_play_records_frames(tmp_path, monkeypatch):
    from quadrupedal_agility_amd import render
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.scripts import play as play_mod
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    from tests.test_render_cpu import _decode_png
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = 256; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False
    t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = False
    args = get_args(["--device", "gpu", "--terrain", "plane"])
    env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=str(tmp_path / "run"))
    runner.learn(2, init_at_random_ep_len=True)
    del env, runner
    frames = tmp_path / "frames"
    first = []
    capture = render.FrameRecorder.capture

    def spy(self, i):
        if i == 0:
            first.append(self.render().cpu().numpy().copy())
        return capture(self, i)
    monkeypatch.setattr(render.FrameRecorder, "capture", spy)
    monkeypatch.setattr(sys, "argv", ["play.py", "--device", "gpu", "--terrain", "plane", "--log_root", str(tmp_path / "run"), "--num_steps", "6", "--record_frames",
                                      str(frames), "--record_every", "2", "--frame_size", "64x48", "--num_envs", "4"])
    env_cfg, _ = task_registry.get_cfgs(name="go2_locomotion")
    try:
        play_mod._main()
    finally:
        if hasattr(env_cfg.sim.qa, "export_body_state"):
            del env_cfg.sim.qa.export_body_state          # the registry's config object is shared by the tests of one process
    assert sorted(os.listdir(frames)) == ["0.png", "1.png", "2.png"]
    imgs = [_decode_png(open(frames / f"{i}.png", "rb").read()) for i in range(3)]
    assert all(im.shape == (48, 64, 3) for im in imgs)
    assert len(first) == 1 and np.array_equal(imgs[0], first[0][0])
    assert len({im.tobytes() for im in imgs}) > 1                     # the robot moves


def test_course_env_frame_shows_floor_and_ceiling():
    from quadrupedal_agility_amd.render import FrameRecorder
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    env = lr.LeggedRobot(make_cfg(4, 3), sim_device="cuda:0")
    q = env.sim.cfg
    cm = env.sim.t["CEILING_SAMPLES"].cpu().numpy(); hm = env.sim.t["HEIGHT_SAMPLES"].cpu().numpy()
    cells = np.argwhere(cm != rr.NO_CEILING)
    assert len(cells) > 0
    i, j = cells[len(cells) // 2]
    x, y, zc = i * q.hf_hscale - q.hf_border, j * q.hf_hscale - q.hf_border, cm[i, j] * q.hf_vscale
    ie = max(int(i - 1.5 / q.hf_hscale), 0)
    eye = (ie * q.hf_hscale - q.hf_border, y, hm[ie, j] * q.hf_vscale + 0.35)       # 1.5 m in front of a bar / tyre / roof cell, below its height
    rec = FrameRecorder(env, "unused", env_ids=(0,), size=(64, 48), camera="fixed", eye=eye, target=(x, y, zc), with_ids=True)
    rgb = rec.render()
    torch.cuda.synchronize()
    ids = set(np.unique(rec.ids.cpu().numpy()).tolist())
    assert rgb.shape == (1, 48, 64, 3) and {19, 20} <= ids, ids
    # and, once a step has written RIGID_BODY_STATE, the follow camera sees the robot on the course
    env.step(torch.zeros(env.num_envs, 12, device=env.device))
    from quadrupedal_agility_amd.render import COURSE_OFFSET
    rec = FrameRecorder(env, "unused", env_ids=(0, 3), size=(64, 48), with_ids=True, fov_deg=30, offset=COURSE_OFFSET)
    rec.render()
    seen = rec.ids.cpu().numpy()
    assert all(((seen[k] >= 0) & (seen[k] < 19)).any() for k in range(2))
    # the reference's camera_pos_bias stands behind the lane's 2 m wall there: floor only (what tests/render_ref.py gives on these maps too)
    rec = FrameRecorder(env, "unused", env_ids=(0,), size=(64, 48), with_ids=True, fov_deg=20)
    rec.render()
    assert set(np.unique(rec.ids.cpu().numpy()).tolist()) == {19}


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_return_qa_e_arg_and_touch_nothing():
    import ctypes as C
    lib = _capi.load_library()
    dev = "cuda:0"
    n, K, Hh, Ww = 3, 2, 8, 8
    body = torch.zeros(n, 19, 13, device=dev); body[..., 6] = 1
    env_ids = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    cams = torch.tensor([[0, -2, 1, 0, 0, 0, 1.0]] * 2, device=dev)
    rgb = torch.full((K, Hh, Ww, 3), SENTINEL_U8, dtype=torch.uint8, device=dev)
    depth = torch.full((K, Hh, Ww), SENTINEL_F32, device=dev); ids = torch.full((K, Hh, Ww), SENTINEL_I8, dtype=torch.int8, device=dev)
    hm = torch.zeros(4, 4, dtype=torch.int16, device=dev)

    def call(**over):
        cfg, io = _capi.QaRenderCfg(), _capi.QaRenderIo()
        cfg.num_envs, cfg.num_cameras, cfg.width, cfg.height, cfg.far, cfg.flags = n, K, Ww, Hh, 10.0, 3
        cfg.light_dir[2] = 1.0
        io.body_state, io.env_ids, io.cameras, io.rgb, io.depth, io.ids = (x.data_ptr() for x in (body, env_ids, cams, rgb, depth, ids))
        for k, v in over.items():
            setattr(cfg if hasattr(cfg, k) else io, k, v)
        return lib.qa_render_frames(C.byref(cfg), C.byref(io), _capi.stream(rgb))
    bad_ids = torch.tensor([0, 3], dtype=torch.int32)
    cases = [dict(num_cameras=0), dict(width=0), dict(height=0), dict(width=40000, height=40000), dict(rgb=None), dict(body_state=None),
             dict(env_ids_host=bad_ids.data_ptr()), dict(terrain_type=1), dict(terrain_type=1, height_samples=hm.data_ptr(), map_rows=4, map_cols=4),
             dict(terrain_type=2), dict(far=0.0)]
    for over in cases:
        assert call(**over) == -1, over
        assert b"qa_render_frames" in lib.qa_last_error()
    torch.cuda.synchronize()
    assert (rgb == SENTINEL_U8).all() and (depth == SENTINEL_F32).all() and (ids == SENTINEL_I8).all()
    assert call() == 0                                               # and the same call without an error renders
    torch.cuda.synchronize()
    assert (ids != SENTINEL_I8).all()
    from quadrupedal_agility_amd.render import render_frames
    with pytest.raises(ValueError):
        render_frames(body, env_ids.long(), cams, rgb)
    with pytest.raises(RuntimeError, match="outside"):
        render_frames(body, env_ids, cams, rgb, env_ids_host=bad_ids)
