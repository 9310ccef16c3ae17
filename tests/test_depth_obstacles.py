"""-m gpu: qa_tsc_depth_update_obstacles (include/qa_tsc_depth_obstacles.h) -- the depth ray-cast with the see-saw, bar and
tyre in their current joint state.  Without records it is qa_tsc_depth_update bit for bit; with them it reads the closed-form scenes and
agrees with the float64 reference (tests/depth_obstacles_ref.py) on a generated course; the empty-space skipping changes no pixel; the env
passes the engine's live tensors; the recorded vision env step equals the eager one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd import _capi
from quadrupedal_agility_amd.tsc.legged_gym.task_level import coarse_depth_maps
from tests import depth_obstacles_ref as ref
from tests import depth_obstacles_scenes as sc
from tests.test_tsc_depth import HC, WC, depth_cfg, oracle_fn, render

pytestmark = pytest.mark.gpu

SMALL, PRODUCT = (30, 16), (106, 60)                  # 11 x 14 = 154 pixels: one partial tile; 87 x 58 = 5046: 20 tiles, the last one partial


def sized_cfg(n, size, rows, cols, **kw):
    c = depth_cfg(n, rows, cols, **kw)
    c.width, c.height = size
    return c, c.height - 2, c.width - 19


def render_obst(cfg, root, pitch, hmap, cmap, ep, buf, desc=None, state=None, struct=True, coarse=None):
    """qa_tsc_depth_update_obstacles on the current stream; `struct` False passes a NULL struct, desc / state None pass NULL pointers"""
    io = _capi.QaTscDepthIo()
    if coarse is not None:
        cfg.coarse_log2 = 3
        io.coarse_floor_max = coarse[0].data_ptr()
        io.coarse_ceiling_min = coarse[1].data_ptr() if coarse[1] is not None else None
    io.root_states, io.camera_pitch, io.height_samples = root.data_ptr(), pitch.data_ptr(), hmap.data_ptr()
    io.ceiling_samples = cmap.data_ptr() if cmap is not None else None
    io.episode_length, io.depth_buffer = ep.data_ptr(), buf.data_ptr()
    ob = _capi.QaTscDepthObstacles(desc.data_ptr() if desc is not None else None, state.data_ptr() if state is not None else None)
    rc = _capi.load_library().qa_tsc_depth_update_obstacles(C.byref(cfg), C.byref(io), C.byref(ob) if struct else None,
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, _capi.load_library().qa_last_error())
    return buf


def course_gpu(n):
    c = sc.course()
    g = {k: c[k][:n].contiguous().cuda() for k in ("root", "pitch", "ep", "desc", "state")}
    g["hmap"], g["cmap"] = c["hmap"].cuda(), c["cmap"].cuda()
    g["coarse"] = coarse_depth_maps(g["hmap"], g["cmap"], 3)
    return g


def maps_args(g):
    return g["root"], g["pitch"], g["hmap"], g["cmap"], g["ep"]


# ------------------------------------------------------------------ off is off
@pytest.mark.parametrize("n,size", [(3, SMALL), (9, SMALL), (3, PRODUCT)])
def test_without_records_it_is_the_static_render_bit_for_bit(n, size):
    """9 envs = two XCD slots with seven padding workgroups that leave before the barrier; 154 pixels = a tile whose idle lanes must reach it.
    Noise on, a non-trivial previous ring, both ring modes (episode_length <= 1 fills, else shifts)"""
    g = course_gpu(n)
    rows, cols = g["hmap"].shape
    kw = dict(noise=0.05, step=11, seed=3, border=5.0)
    cfg, hc, wc = sized_cfg(n, size, rows, cols, **kw)
    assert (g["ep"] <= 1).any() and (g["ep"] > 1).any()
    start = torch.randn(n, 2, hc, wc, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    want = start.clone()
    render(_capi.load_library().qa_tsc_depth_update, cfg, *maps_args(g), want, st, coarse=g["coarse"])
    none = g["desc"].clone(); none[:, :, 7] = 0
    far = g["desc"].clone(); far[:, :, :2] += 40.0
    variants = dict(null_struct=dict(struct=False), null_pointers=dict(), kind_zero=dict(desc=none, state=g["state"]),
                    far_away=dict(desc=far, state=g["state"]))
    for name, v in variants.items():
        got = render_obst(sized_cfg(n, size, rows, cols, **kw)[0], *maps_args(g), start.clone(), coarse=g["coarse"], **v)
        torch.cuda.synchronize()
        diff = (got - want).abs()
        print(f"{name}: {int((diff > 0).sum())} of {diff.numel()} ring entries differ from qa_tsc_depth_update's, max {diff.max().item():.2e}")
        assert torch.equal(got, want), name
    live = render_obst(sized_cfg(n, size, rows, cols, **kw)[0], *maps_args(g), start.clone(), g["desc"], g["state"], coarse=g["coarse"])
    torch.cuda.synchronize()
    assert not torch.equal(live, want)
    # ring and noise do not depend on the records: old frame shifted down, or all slots = the new image
    fill = g["ep"] <= 1
    assert torch.equal(live[~fill][:, 0], start[~fill][:, 1]) and torch.equal(live[fill][:, 0], live[fill][:, 1])


# ------------------------------------------------------------------ closed-form scenes
@pytest.mark.parametrize("yaw", sc.SEESAW_YAWS)
def test_hip_reads_the_planks_top_plane(yaw):
    """three envs, one per tilt (both stops and 0.05 rad): HIP against the closed-form depth at 1e-4 of the normalised range (the bound the
    course test of tests/test_tsc_depth.py holds HIP to against float64), on the pixels tests/test_depth_obstacles_cpu.py keeps"""
    root, pitch, hmap, ep = sc.flat_scene()
    recs = [sc.seesaw_record(root, yaw, q) for q in sc.SEESAW_TILTS]
    desc = torch.from_numpy(np.concatenate([r[0] for r in recs])).cuda(); state = torch.from_numpy(np.concatenate([r[1] for r in recs])).cuda()
    n = 3
    buf = torch.zeros(n, 2, HC, WC, device="cuda")
    hm = hmap.cuda()
    for coarse in (None, coarse_depth_maps(hm, None, 3)):
        render_obst(depth_cfg(n, 200, 200), root.repeat(n, 1).cuda(), pitch.repeat(n).cuda(), hm, None, ep.repeat(n).cuda(), buf, desc, state, coarse=coarse)
        torch.cuda.synchronize()
        for e, q in enumerate(sc.SEESAW_TILTS):
            t, plank, keep = sc.seesaw_analytic(root, *recs[e], WC, HC)
            err = np.abs(buf[e, -1].cpu().numpy() - sc.norm(t))[keep]
            print(f"yaw {yaw} q {q:+.3f} coarse {coarse is not None}: {keep.sum()} pixels, max error {err.max():.2e}")
            assert keep.sum() > 400 and err.max() < 1e-4


def test_hip_lifts_a_box_under_a_bar_record_by_q():
    qs = (0.03, -0.03, 0.0)
    scenes = [sc.bar_scene(q) for q in qs]
    root, pitch, hmap, ep = scenes[0][:4]
    desc = torch.from_numpy(np.concatenate([s[4] for s in scenes])).cuda(); state = torch.from_numpy(np.concatenate([s[5] for s in scenes])).cuda()
    n = 3
    buf = torch.zeros(n, 2, HC, WC, device="cuda")
    render_obst(depth_cfg(n, 200, 200), root.repeat(n, 1).cuda(), pitch.repeat(n).cuda(), hmap.cuda(), None, ep.repeat(n).cuda(), buf, desc, state)
    torch.cuda.synchronize()
    for e, q in enumerate(qs):
        t, keep = sc.bar_analytic(root, scenes[e][5], WC, HC)
        err = np.abs(buf[e, -1].cpu().numpy() - sc.norm(t))[keep]
        print(f"bar q {q:+.3f}: {keep.sum()} pixels, max error {err.max():.2e}")
        assert keep.sum() > 150 and err.max() < 1e-4


# ------------------------------------------------------------------ a generated course
N_COURSE = 16


@functools.lru_cache(maxsize=None)
def course_reference():
    """computed once: the float64 images with and without the records (clean), and the additive noise field of the key (seed 3; env, step 11)
    -- the oracle's static render with noise less the one without; both store fp32, so the field is good to 1.2e-7"""
    c = sc.course()
    n = N_COURSE
    rows, cols = c["hmap"].shape
    cfg = depth_cfg(n, rows, cols, border=5.0)
    args = (cfg, c["root"].numpy(), c["pitch"].numpy(), c["hmap"].numpy(), c["cmap"].numpy())
    live, static = ref.render(*args, c["desc"].numpy(), c["state"].numpy()), ref.render(*args)
    b = {}
    for noise in (0.0, 0.05):
        b[noise] = torch.zeros(n, 2, HC, WC)
        render(oracle_fn(), depth_cfg(n, rows, cols, noise=noise, step=11, seed=3, border=5.0), c["root"], c["pitch"], c["hmap"], c["cmap"], c["ep"], b[noise])
    return dict(live=live, static=static, noise=(b[0.05][:, -1] - b[0.0][:, -1]).numpy().astype(np.float64))


def test_hip_matches_the_float64_reference_on_a_course():
    """cameras within 2 m of the see-saws, bars and tyres of a 16-env course, facing them, the joints anywhere between their stops (both
    extremes included): pixels off by more than 1e-4 stay under 1 %, and the noise adds no disagreement (the bounds of
    test_hip_depth_matches_oracle_on_a_course)"""
    g, r = course_gpu(N_COURSE), course_reference()
    n = N_COURSE
    rows, cols = g["hmap"].shape
    start = torch.randn(n, 2, HC, WC)
    ep = g["ep"].cpu().numpy()
    off = {}
    for noise in (0.0, 0.05):
        got = render_obst(depth_cfg(n, rows, cols, noise=noise, step=11, seed=3, border=5.0), *maps_args(g), start.clone().cuda(), g["desc"], g["state"], coarse=g["coarse"])
        torch.cuda.synchronize()
        want = ref.push(start.numpy().astype(np.float64), r["live"] + (r["noise"] if noise else 0.0), ep)
        d = np.abs(got.cpu().numpy() - want)
        off[noise] = (d > 1e-4).mean()
        print(f"noise {noise}: pixels off by > 1e-4: {off[noise]:.4%}, median {np.median(d):.2e}, seen-something fraction {(np.abs(r['live']) < 0.499).mean():.2f}")
        assert off[noise] < 0.01
        assert np.array_equal((got[:, 0] == got[:, 1]).flatten(1).all(1).cpu().numpy(), ep <= 1)
    assert off[0.05] <= off[0.0] + 1e-4


def test_the_moving_parts_are_visible():
    """in the envs that face a see-saw at least 5 % of the pixels differ from the static render by more than 1e-3 (the float64 reference
    shows 9.8 % .. 25 % for these placements)"""
    g, r = course_gpu(N_COURSE), course_reference()
    n = N_COURSE
    rows, cols = g["hmap"].shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    static = torch.zeros(n, 2, HC, WC, device="cuda")
    render(_capi.load_library().qa_tsc_depth_update, depth_cfg(n, rows, cols, border=5.0), *maps_args(g), static, st, coarse=g["coarse"])
    live = render_obst(depth_cfg(n, rows, cols, border=5.0), *maps_args(g), torch.zeros(n, 2, HC, WC, device="cuda"), g["desc"], g["state"], coarse=g["coarse"])
    torch.cuda.synchronize()
    share = ((live[:, -1] - static[:, -1]).abs() > 1e-3).float().flatten(1).mean(1).cpu().numpy()
    want = (np.abs(r["live"] - r["static"]) > 1e-3).reshape(n, -1).mean(1)
    for e in range(0, n, 3):
        print(f"env {e} (see-saw at q = {g['state'][e, 0, 0].item():+.3f}): {share[e]:.1%} of the pixels differ from the static render (float64: {want[e]:.1%})")
    assert (want[0::3] >= 0.05).all() and (share[0::3] >= 0.05).all()


@pytest.mark.parametrize("n,size", [(16, PRODUCT), (9, SMALL)])
def test_skipping_changes_no_pixel(n, size):
    """the coarse maps bound the static map only; blocks that overlap a footprint's box are never skipped, so the image with the coarse
    pointers is the full march's.  The course holds a see-saw at each stop (envs 0, 3), a bar at +0.05 m -- above anything the coarse map
    knows (env 1) -- and a tyre at -0.05 m (env 5)"""
    g = course_gpu(n)
    s = g["state"].cpu()
    assert s[0, 0, 0] == sc.MAX_TILT and s[3, 0, 0] == -sc.MAX_TILT and s[1, 1, 0] == np.float32(0.05) and s[5, 2, 0] == np.float32(-0.05)
    rows, cols = g["hmap"].shape
    kw = dict(noise=0.05, step=4, seed=2, border=5.0)
    cfg, hc, wc = sized_cfg(n, size, rows, cols, **kw)
    start = torch.randn(n, 2, hc, wc, device="cuda")
    skip = render_obst(cfg, *maps_args(g), start.clone(), g["desc"], g["state"], coarse=g["coarse"])
    full = render_obst(sized_cfg(n, size, rows, cols, **kw)[0], *maps_args(g), start.clone(), g["desc"], g["state"])
    torch.cuda.synchronize()
    assert torch.equal(skip, full)


def test_one_null_pointer_is_refused_before_anything_is_launched():
    g = course_gpu(3)
    rows, cols = g["hmap"].shape
    cfg = depth_cfg(3, rows, cols, border=5.0)
    buf = torch.full((3, 2, HC, WC), 7.0, device="cuda")
    io = _capi.QaTscDepthIo()
    io.root_states, io.camera_pitch, io.height_samples, io.ceiling_samples = (g[k].data_ptr() for k in ("root", "pitch", "hmap", "cmap"))
    io.episode_length, io.depth_buffer = g["ep"].data_ptr(), buf.data_ptr()
    for ob in (_capi.QaTscDepthObstacles(g["desc"].data_ptr(), None), _capi.QaTscDepthObstacles(None, g["state"].data_ptr())):
        with pytest.raises(RuntimeError, match="obst_desc and obst_state"):
            _capi.API.launch("tsc_depth_update_obstacles", C.byref(cfg), C.byref(io), C.byref(ob), on=buf)
    torch.cuda.synchronize()
    assert (buf == 7.0).all()


# ------------------------------------------------------------------ the env
def _camera_env(flag, flip):
    """4 camera envs; robot 0 stands 1 m in front of its see-saw's near end, facing it; `flip` writes the opposite stop before the step"""
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    torch.manual_seed(0)
    # (leave_goal_threshold: the robot is moved away from its current goal by hand; the default 4 m would end its episode)
    env = lr.LeggedRobot(make_cfg(4, 5, depth__use_camera=True, depth__qa_articulated=flag, env__leave_goal_threshold=1e3), sim_device="cuda:0")
    d = env.sim.t["OBST_DESC"][0, 0].cpu().numpy()
    psi = np.arctan2(d[3], d[2])
    hm = env.height_samples.cpu().numpy()
    ground = lambda x, y: 0.005 * float(hm[int((x + 5.0) / 0.05), int((y + 5.0) / 0.05)])          # noqa: E731
    x0, y0, z0 = (float(v) for v in env.root_states[0, :3])
    x1, y1 = float(d[0] - 2.5 * d[2]), float(d[1] - 2.5 * d[3])
    env.root_states[0, 0], env.root_states[0, 1], env.root_states[0, 2] = x1, y1, z0 - ground(x0, y0) + ground(x1, y1)
    env.root_states[0, 3:7] = torch.tensor([0.0, 0.0, np.sin(psi / 2), np.cos(psi / 2)], device=env.root_states.device)
    env.root_states[0, 7:] = 0
    if flip:
        env.obst_state[:, 0, 0] = -env.obst_state[:, 0, 0]
    env.step(torch.zeros(4, 12, device="cuda:0"))
    torch.cuda.synchronize()
    return env


def test_env_renders_the_live_joint_state():
    on, on_flipped = _camera_env(True, False), _camera_env(True, True)
    assert on.bk._depth_obst[0].data_ptr() == on.sim.t["OBST_DESC"].data_ptr() and on.bk._depth_obst[1].data_ptr() == on.obst_state.data_ptr()
    print("robot 0 after the step: reset", on.bk.reset_buf[0].item(), on_flipped.bk.reset_buf[0].item(), "root", on.root_states[0, :7].tolist())
    assert on.bk.reset_buf[0] == 0 and on_flipped.bk.reset_buf[0] == 0
    assert torch.equal(on.root_states[0], on_flipped.root_states[0])                       # the robot is not on the plank: same physics
    share = ((on.depth_buffer[0, -1] - on_flipped.depth_buffer[0, -1]).abs() > 1e-3).float().mean().item()
    print(f"see-saw at the other stop: {share:.1%} of robot 0's newest image changes")
    assert share > 0.05
    off, off_flipped = _camera_env(False, False), _camera_env(False, True)
    assert off.bk._depth_obst is None and torch.equal(off.depth_buffer, off_flipped.depth_buffer)
    assert not torch.equal(off.depth_buffer[0, -1], on.depth_buffer[0, -1])


def test_recorded_vision_env_step_equals_the_eager_one_with_the_flag_on(tmp_path, monkeypatch):
    """the protocol of tests/test_tsc_depth.py::test_recorded_vision_env_step_equals_the_eager_one with depth.qa_articulated: the recorded env
    step captures qa_tsc_depth_update_obstacles, which reads device tensors only -- root, images and observations equal the eager run's bit
    for bit.  learn() is entered twice; depth.update_interval 2 records both camera phases"""
    import random
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    from tests.test_tsc_depth import _vision_runner
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("QA_TSC_ROLLOUT_GRAPH", mode)
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = make_cfg(64, 1, env__episode_length_s=1.0, depth__use_camera=True, depth__update_interval=2, depth__qa_articulated=True)
        env = lr.LeggedRobot(cfg, sim_device="cuda:0")
        assert env.bk._depth_obst is not None
        runner = _vision_runner(env, tmp_path / mode, "cuda:0", steps=12)
        runner.log_dir = None
        for k in (2, 1):
            runner.learn(k)
        torch.cuda.synchronize()
        if mode == "1":
            gr = runner._vs["graphs"]
            assert set(gr) == {False, True} and all(v is not False for v in gr.values()), gr          # both camera phases were recorded
        res[mode] = dict(root=env.root_states.clone(), depth=env.depth_buffer.clone(), obs=env.get_observations().clone(), q=env.obst_state.clone())
    a, b = res["0"], res["1"]
    assert torch.equal(a["root"], b["root"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["obs"], b["obs"]) and torch.equal(a["q"], b["q"])
