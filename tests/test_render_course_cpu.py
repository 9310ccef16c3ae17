"""The course mode of the frame renderer without a GPU: the float64 reference tests/render_course_ref.py against closed forms on a flat map,
its own edge-pixel share on the scenes the GPU tests use, the host twin of csrc/qa_render_course_walk.h against it, and the Python plumbing
(argument checks, recorder options, command-line flags of both trees)."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import render_course_ref as rc
from tests import render_course_scenes as cs
from tests import render_ref as rr
from tests import render_scenes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernel's own bound (tests/test_render.py): the twin is the same fp32 code, run by the host
DEPTH_REL_TOL = 4 * 1.211e-6
EDGE_CAP = 0.01


# ------------------------------------------------------------------ the reference against closed forms on a flat map
def _flat(desc, state, cam, goals=None, **kw):
    hm = np.zeros((rs.ROWS, rs.COLS), np.int16)
    s = cs._scene(rs.parked_rows()[None], [0], [cam], hm, far=20.0, width=48, height=32, obst_desc=np.asarray(desc)[None], obst_state=np.asarray(state)[None], **kw)
    if goals is not None:
        s.update(goals=rs._f32(goals)[None], cur_goal_idx=[0], reached=[0], goal_radius=0.1)
    s["table"], s["palette"] = [dict(kind=rr.SPHERE, body=0, cls=0, a=(0, 0, 0), b=(0, 0, 0), r=0.01)], [(0.5, 0.5, 0.5)] * 8
    return s


@pytest.mark.parametrize("yaw", [0.0, 0.6])
@pytest.mark.parametrize("q", [cs.MAX_TILT, -cs.MAX_TILT, 0.05])
def test_reference_plank_is_its_top_plane(q, yaw):
    desc = [cs._desc(4.0, 4.0, yaw, 1.5, 0.3, 0.26, cs.SEESAW), [0] * 8, [0] * 8]
    state = [cs._state(q), [0] * 4, [0] * 4]
    scene = _flat(desc, state, rs.camera((3.7, 3.2, 2.9), (4.0, 4.0, 0.2), 50.0))
    c = rc.trace(scene, 0)
    o, d = rr.camera_rays(scene["cameras"][0], 48, 32)
    d32 = np.asarray(scene["obst_desc"][0, 0]); q32 = float(scene["obst_state"][0, 0, 0])
    nrm = np.array([d32[2] * np.sin(q32), d32[3] * np.sin(q32), np.cos(q32)])          # lx sin q + (z - h0) cos q = 0
    p0 = np.array([d32[0], d32[1], d32[6]])
    tp = ((p0 - o) @ nrm) / (d @ nrm)
    on = c["ids"] == rc.ID_OBSTACLE
    assert on.sum() > 100
    assert np.abs(c["depth"][on] - tp[on]).max() < 1e-9
    hit = o + c["depth"][:, None] * d
    assert (hit[on, 2] > 0).all() and hit[on, 2].max() > 0.26 + 1.4 * np.tan(abs(q32)) * 0.8       # up to near the high end
    # inside the footprint where the plank is below 0, and outside: the ground at 0
    gr = c["ids"] == rr.ID_GROUND
    assert gr.sum() > 100 and np.abs(hit[gr, 2]).max() < 1e-9
    if abs(q) > 0.1:                                                                      # the far long side is hidden; a near one shows its face
        assert (c["ids"] == rc.ID_SIDE).any()


@pytest.mark.parametrize("q", [0.05, -0.05])
def test_reference_shifted_block_top_and_side_face(q):
    """a block of 0.5 m under a bar's footprint (yaw 0, edges off the lattice) shifted by q: its top at 0.5 + q, the ground inside the
    footprint at q, and the face at the footprint's near edge x = 2.6 between them"""
    hm = np.zeros((rs.ROWS, rs.COLS), np.int16); hm[20:24, 18:22] = 100            # x 3.0 .. 3.75, y 2.5 .. 3.25 (+ one cell of slope around)
    desc = [[0] * 8, cs._desc(3.5, 3.0, 0.0, 0.9, 1.1, 0.0, cs.BAR), [0] * 8]
    state = [[0] * 4, cs._state(q), [0] * 4]
    scene = _flat(desc, state, rs.camera((0.5, 2.9, 1.5), (3.4, 3.0, 0.3), 40.0))
    scene["terrain"]["height_samples"] = hm
    c = rc.trace(scene, 0)
    o, d = rr.camera_rays(scene["cameras"][0], 48, 32)
    q32 = float(scene["obst_state"][0, 1, 0])
    hit = o + c["depth"][:, None] * d
    top = (c["ids"] == rc.ID_OBSTACLE) & (hit[:, 0] > 3.05) & (hit[:, 0] < 3.7) & (np.abs(hit[:, 1] - 2.875) < 0.3)
    block = 100 * float(scene["terrain"]["vertical_scale"])                              # (the fp32 scale's 0.5)
    assert top.sum() > 20 and np.abs(hit[top, 2] - (block + q32)).max() < 1e-9
    inside = (c["ids"] == rc.ID_OBSTACLE) & (hit[:, 0] < 2.7)
    outside = (c["ids"] == rr.ID_GROUND)
    assert np.abs(hit[outside, 2]).max() < 1e-9 and (hit[outside, 0] < 2.6 + 1e-9).any()
    side = c["ids"] == rc.ID_SIDE
    if q > 0:                   # raised: the step of q faces the camera at x = 2.6
        assert side.sum() > 5 and np.abs(hit[side, 0] - 2.6).max() < 1e-6 and (hit[side, 2] >= -1e-9).all() and (hit[side, 2] <= q32 + 1e-9).all()
        assert np.abs(c["depth"][side] - (2.6 - o[0]) / d[side, 0]).max() < 1e-6
        assert inside.sum() > 5 and np.abs(hit[inside, 2] - q32).max() < 1e-9
    else:                       # lowered: a pit; its far wall (leaving the footprint at x = 4.4) and its side walls face the camera
        assert side.sum() > 5 and (hit[side, 2] <= 1e-9).all() and (hit[side, 2] >= q32 - 1e-9).all()
        far_wall = side & (np.abs(hit[:, 0] - 4.4) < 1e-6)
        assert far_wall.any()


def test_reference_goal_sphere():
    desc, state = [[0] * 8] * 3, [[0] * 4] * 3
    centre = np.array([3.0, 3.0, 0.05])                                                 # half sunk: the floor cuts it
    scene = _flat(desc, state, rs.camera((1.0, 2.0, 0.35), (3.0, 3.0, 0.1), 12.0), goals=[centre, (50.0, 50.0, 1.0)])
    c = rc.trace(scene, 0)
    o, d = rr.camera_rays(scene["cameras"][0], 48, 32)
    oc = o - rs._f32(centre)
    b = d @ oc; disc = b * b - (oc @ oc - 0.1 ** 2)
    ts = -b - np.sqrt(np.where(disc > 0, disc, np.nan))
    on = c["ids"] == rc.ID_GOAL_CURRENT
    assert on.sum() > 30 and set(np.unique(c["ids"]).tolist()) == {rr.ID_SKY, rr.ID_GROUND, rc.ID_GOAL_CURRENT}
    assert np.abs(c["depth"][on] - ts[on]).max() < 1e-9
    hit = o + c["depth"][:, None] * d
    assert (hit[on, 2] >= -1e-12).all()                                                   # below the floor the ground is nearer
    under = np.isfinite(ts) & ((o + ts[:, None] * d)[:, 2] < 0)
    assert under.any() and (c["ids"][under] == rr.ID_GROUND).all()
    col = rc.constants()["COLOURS"][rc.ID_GOAL_CURRENT]
    assert col == (0.0, 0.0, 1.0) and (c["rgb"][on][:, :2] == 0).all()


def test_header_constants_are_the_reference_ids():
    k = rc.constants()
    assert (k["ID_OBSTACLE"], k["ID_SIDE"], k["ID_GOAL"], k["ID_GOAL_CURRENT"], k["ID_GOAL_REACHED"]) == (21, 22, 23, 24, 25)
    assert k["COLOURS"][23] == (1.0, 0.0, 0.0) and k["COLOURS"][25] == (0.0, 1.0, 0.0) and k["COLOURS"][21] == k["COLOURS"][22]


# ------------------------------------------------------------------ the reference alone on the scenes the GPU tests use
@pytest.mark.parametrize("name", sorted(cs.SCENES))
def test_reference_flags_few_edge_pixels_and_no_hit_on_a_checker_line(name):
    import __graft_entry__ as g
    g.build()
    scene = cs.scene(name)
    seen = set()
    for k in range(len(scene["env_ids"])):
        ids, depth, rgb, edge = cs.reference(name, k)
        share = float(edge.mean())
        print(f"{name} camera {k}: edge share {share:.4%}, ids {sorted(set(ids.ravel().tolist()))}")
        assert share <= 0.005, (name, k, share)
        seen |= set(ids.ravel().tolist())
        o, d = rr.camera_rays(scene["cameras"][k], scene["width"], scene["height"])
        hp = (o + depth.ravel()[:, None] * d)[ids.ravel() == rr.ID_GROUND, :2] / rr.CHECKER_SIZE
        assert hp.size == 0 or (np.abs(hp - np.round(hp)).min() * rr.CHECKER_SIZE > 2e-5), (name, k)
    want = dict(seesaw={19, 21, 22}, bar_tyre={19, 20, 21, 22}, bar_tyre_61x35={19, 20, 21, 22}, goals={19, 23, 24, 25}, static={19})[name]
    assert want <= seen, (name, sorted(seen))


# ------------------------------------------------------------------ the host twin of csrc/qa_render_course_walk.h
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("rcourse") / "libqa_render_course_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "c_host", "qa_render_course_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qa_render_course_host.restype = C.c_int
    lib.qa_render_course_host.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 2 +
                                          [C.c_int] * 3 + [C.c_void_p] * 3)
    return lib


def host_render(lib, scene, k):
    e = int(scene["env_ids"][k])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    body, cam = f32(scene["body_state"][e]), f32(scene["cameras"][k])
    desc = f32(scene["obst_desc"][e]) if scene.get("obst_desc") is not None else None
    state = f32(scene["obst_state"][e]) if desc is not None else None
    goals = f32(scene["goals"][e]) if scene.get("goals") is not None else None
    t = scene["terrain"]
    hm = np.ascontiguousarray(t["height_samples"]); cm = np.ascontiguousarray(t["ceiling_samples"]) if t.get("ceiling_samples") is not None else None
    geo = f32([t["border_size"], t["horizontal_scale"], t["vertical_scale"], scene["far"]])
    light = np.asarray(scene["light_dir"], np.float64); light = f32(light / np.linalg.norm(light))
    Wd, Hd = scene["width"], scene["height"]
    rgb, depth, ids = np.zeros((Hd, Wd, 3), np.uint8), np.zeros((Hd, Wd), np.float32), np.zeros((Hd, Wd), np.int8)
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc_ = lib.qa_render_course_host(ptr(body), ptr(desc), ptr(state), ptr(goals), 0 if goals is None else goals.shape[0], float(scene.get("goal_radius", 0.1)),
                                    int(scene["cur_goal_idx"][e]) if goals is not None else -1, int(scene["reached"][e]) if goals is not None else 0,
                                    ptr(cam), ptr(hm), ptr(cm), hm.shape[0], hm.shape[1], ptr(geo), ptr(light), int(scene["flags"]), Wd, Hd,
                                    ptr(rgb), ptr(depth), ptr(ids))
    assert rc_ == 0
    return ids.astype(np.int64), depth.astype(np.float64), rgb


def compare_camera(name, k, ids, depth, rgb, tol):
    """test_render.py's rule for one camera: ids equal, colours within one level, edge pixels (at most 1 %) excluded; returns the depth error"""
    rid, rdepth, rrgb, edge = cs.reference(name, k)
    assert edge.mean() <= EDGE_CAP, (name, k, edge.mean())
    ok = ~edge
    bad = ok & (ids != rid)
    assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:5].tolist(), ids[bad][:5], rid[bad][:5])
    err = float((np.abs(depth - rdepth) / np.maximum(1.0, rdepth))[ok].max())
    diff = np.abs(rgb.astype(np.int64) - rrgb.astype(np.int64)).max(axis=-1)
    print(f"{name} camera {k}: edge share {edge.mean():.4%}, depth rel err {err:.3e}, rgb off by one level {float((diff[ok] > 0).mean()):.4%}, "
          f"ids {sorted(set(rid.ravel().tolist()))}")
    assert err <= tol, (name, k, err)
    assert diff[ok].max() <= 1, (name, k, int(diff[ok].max()), np.argwhere(ok & (diff > 1))[:5].tolist())
    return err


@pytest.mark.parametrize("name", sorted(cs.SCENES))
def test_host_twin_matches_the_reference(twin, name):
    import __graft_entry__ as g
    g.build()
    scene = cs.scene(name)
    for k in range(len(scene["env_ids"])):
        compare_camera(name, k, *host_render(twin, scene, k), DEPTH_REL_TOL)


# ------------------------------------------------------------------ Python plumbing
class _SpyApi:
    def __init__(self):
        self.launches = []

    def launch(self, name, *args, on):
        self.launches.append(name)


def _args(n=3, k=2, g=4):
    body = torch.zeros(n, 19, 13); body[..., 6] = 1
    return dict(body_state=body, env_ids=torch.tensor([0, 2], dtype=torch.int32), cameras=torch.zeros(k, 7), rgb=torch.zeros(k, 8, 8, 3, dtype=torch.uint8),
                height_samples=torch.zeros(4, 4, dtype=torch.int16), horizontal_scale=0.25, vertical_scale=0.005,
                obst_desc=torch.zeros(n, 3, 8), obst_state=torch.zeros(n, 3, 4), goals=torch.zeros(n, g, 3), cur_goal_idx=torch.zeros(n, dtype=torch.long),
                reached=torch.zeros(n, dtype=torch.uint8))


def test_python_argument_checks_raise_before_any_launch():
    from quadrupedal_agility_amd import _capi, render
    spy = _SpyApi()
    bad = [dict(obst_state=None), dict(obst_desc=None), dict(obst_desc=torch.zeros(3, 1, 8)), dict(obst_state=torch.zeros(3, 3, 4, dtype=torch.float64)),
           dict(goals=torch.zeros(3, 33, 3)), dict(goals=torch.zeros(3, 0, 3)), dict(goals=torch.zeros(2, 4, 3)), dict(goal_radius=0.0),
           dict(cur_goal_idx=torch.zeros(3, dtype=torch.int32)), dict(reached=torch.zeros(3, dtype=torch.bool)), dict(goals=None),
           dict(height_samples=None), dict(reached=torch.zeros(4, dtype=torch.uint8))]
    for over in bad:
        a = _args(); a.update(over)
        with pytest.raises(ValueError):
            render.render_frames(api=spy, **a)
    assert spy.launches == []
    render.render_frames(api=spy, **_args())
    a = _args(); a.update(obst_desc=None, obst_state=None)
    render.render_frames(api=spy, **a)                                       # goals alone
    a = _args(); a.update(goals=None, cur_goal_idx=None, reached=None)
    render.render_frames(api=spy, **a)                                       # obstacles alone
    assert spy.launches == ["render_frames"] * 3
    # the struct and the flag come from the header, not from _capi; the layout is the header's
    assert C.sizeof(render.QaRenderCourse) == C.sizeof(_capi.QaRenderIo) + 5 * 8 + 8 and render.QaRenderCourse.io.offset == 0
    assert render.RENDER_COURSE == 4 and not hasattr(_capi, "QaRenderCourse") and not hasattr(_capi, "RENDER_COURSE")


def test_recorder_options_need_an_env_that_has_them():
    from quadrupedal_agility_amd.render import FrameRecorder
    n = 2
    t = dict(RIGID_BODY_STATE=torch.zeros(n, 19, 13), ROOT_STATES=torch.zeros(n, 13), OBST_DESC=torch.zeros(n, 3, 8))
    sim = types.SimpleNamespace(cfg=types.SimpleNamespace(export_body_state=1, num_envs=n, terrain_type=0), t=t, device=torch.device("cpu"), api=_SpyApi())
    bbc = types.SimpleNamespace(sim=sim)
    FrameRecorder(bbc, "unused")
    for kw in (dict(articulated=True), dict(goals=True)):
        with pytest.raises(ValueError):
            FrameRecorder(bbc, "unused", **kw)
    static = types.SimpleNamespace(sim=sim, articulated=False, env_goals=torch.zeros(n, 26, 3), bk=types.SimpleNamespace(
        cur_goal_idx=torch.zeros(n, dtype=torch.long), reached_goal_ids=torch.zeros(n, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="articulated"):
        FrameRecorder(static, "unused", articulated=True)
    rec = FrameRecorder(static, "unused", goals=True)
    assert rec._opts["goals"] is static.env_goals and rec._opts["cur_goal_idx"] is static.bk.cur_goal_idx and rec._opts["reached"] is static.bk.reached_goal_ids
    live = types.SimpleNamespace(sim=sim, articulated=True, obst_state=torch.zeros(n, 3, 4))
    rec = FrameRecorder(live, "unused", articulated=True)
    assert rec._opts["obst_desc"] is t["OBST_DESC"] and rec._opts["obst_state"] is live.obst_state and "goals" not in rec._opts


def test_record_flags_reach_the_play_configuration_in_both_trees(tmp_path):
    from quadrupedal_agility_amd.legged_gym.utils import helpers as bbc
    from quadrupedal_agility_amd.tsc.legged_gym.utils import helpers as tsc
    from quadrupedal_agility_amd.render import record_settings
    for h in (bbc, tsc):
        base = dict(out_dir=str(tmp_path), env_ids=(0,), size=(640, 360), every=2)
        assert record_settings(h.get_args(["--record_frames", str(tmp_path)]), "exp") == base
        assert record_settings(h.get_args(["--record_frames", str(tmp_path), "--record_articulated"]), "exp") == dict(base, articulated=True)
        assert record_settings(h.get_args(["--record_frames", str(tmp_path), "--record_goals"]), "exp") == dict(base, goals=True)
        assert record_settings(h.get_args(["--record_frames", str(tmp_path), "--record_goals", "--record_articulated"]), "exp") == dict(base, articulated=True, goals=True)
        assert record_settings(h.get_args(["--record_goals"]), "exp") is None
