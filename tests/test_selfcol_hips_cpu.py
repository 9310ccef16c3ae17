"""The calf-against-neighbouring-hip self-collision class (include/qa_sim_selfcol.h) without a GPU: the geometry of
quadrupedal_agility_amd/csrc/qa_selfcol.h -- the functions phys_substep calls -- through the host twin tests/c_host/qa_selfcol_host.cpp
against a float64 closed form (tests/selfcol_hips_ref.py), and the host side: the config translation, the command-line switch, the binding."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi
from tests import selfcol_hips_ref as ref
from tests.test_self_collision import seg_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("sc") / "libqa_selfcol_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "c_host", "qa_selfcol_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qa_selfcol_hip_segment_host.argtypes = [C.c_int] + [C.c_void_p] * 5; lib.qa_selfcol_hip_segment_host.restype = C.c_int
    lib.qa_selfcol_lane_host.argtypes = [C.c_int] + [C.c_void_p] * 10; lib.qa_selfcol_lane_host.restype = C.c_int
    return lib


def sweep_poses():
    """the closest poses the joint-limit sweep found (profiles/self_collision_hips_sweep.json), per ordered front / rear relation"""
    rows = json.load(open(os.path.join(ROOT, "profiles", "self_collision_hips_sweep.json")))["relations"]
    out = []
    for r in rows:
        a, b = ref.LEGS.index(r["calf_leg"]), ref.LEGS.index(r["hip_leg"])
        if (a, b) in ref.RELATIONS:
            out.append((a, b, r["calf_leg_joints_rad"], r["hip_leg_joint0_rad"]))
    return out


@pytest.fixture(scope="module")
def cases():
    """per ordered relation: 2,000 random joint vectors inside the URDF limits + the sweep's closest pose + a band of poses around it (so that
    the set holds deep penetrations, grazing contacts and end-cap contacts, not only legs 20 cm apart); float64 points by the reference FK"""
    rng = np.random.default_rng(11)
    out = []
    for a, b, qa_star, qb0_star in sweep_poses():
        qa = rng.uniform(ref.DOF_LOWER[a], ref.DOF_UPPER[a], (2000, 3))
        qb = rng.uniform(ref.DOF_LOWER[b], ref.DOF_UPPER[b], (2000, 3))
        near_a = np.clip(np.array(qa_star) + rng.uniform(-0.5, 0.5, (400, 3)), ref.DOF_LOWER[a], ref.DOF_UPPER[a])
        near_b = np.clip(np.array([qb0_star, 0.9, -1.8]) + rng.uniform(-0.5, 0.5, (400, 3)), ref.DOF_LOWER[b], ref.DOF_UPPER[b])
        qa = np.concatenate([qa, [qa_star], near_a]); qb = np.concatenate([qb, [[qb0_star, 0.9, -1.8]], near_b])
        gap, n, s, t, pts = ref.calf_hip_gap(qa, a, qb, b)
        out.append(dict(a=a, b=b, qa=qa, qb=qb, gap=gap, n=n, s=s, t=t, pts=pts))
    return out


def run_lane(lib, own0, own1, other0, other1, own_is_calf):
    n = len(own0)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    ins = [f32(own0), f32(own1), f32(other0), f32(other1), np.full(n, int(own_is_calf), np.int32)]
    out = dict(gap=np.zeros(n, np.float32), n=np.zeros((n, 3), np.float32), s=np.zeros(n, np.float32), t=np.zeros(n, np.float32), p=np.zeros((n, 3), np.float32))
    assert lib.qa_selfcol_lane_host(n, *[x.ctypes.data for x in ins], *[out[k].ctypes.data for k in ("gap", "n", "s", "t", "p")]) == 0
    return out


def test_the_sweep_file_says_which_relations_get_a_row():
    """only a front calf reaches the rear hip of its side; every other ordered relation stays outside the contact offset under the limits"""
    rows = json.load(open(os.path.join(ROOT, "profiles", "self_collision_hips_sweep.json")))["relations"]
    assert len(rows) == 12
    for r in rows:
        pair = (ref.LEGS.index(r["calf_leg"]), ref.LEGS.index(r["hip_leg"]))
        assert r["can_touch"] == (pair in ref.ROW_RELATIONS), r
        assert (r["min_gap_m"] < ref.CONTACT_OFFSET) == r["can_touch"]
        # the recorded pose reproduces the recorded gap
        g = ref.calf_hip_gap(np.array(r["calf_leg_joints_rad"]), pair[0], np.array([r["hip_leg_joint0_rad"], 0.0, 0.0]), pair[1])[0]
        assert abs(float(g) - r["min_gap_m"]) < 2e-4, r


def test_closed_form_distance_against_dense_sampling(cases):
    """the float64 closed form itself, pinned to the dense sampling of tests/test_self_collision.py::seg_dist within its sampling step"""
    rng = np.random.default_rng(5)
    for c in cases:
        knee, foot, h0, h1 = c["pts"]
        d = c["gap"] + (ref.CALF_R0 + c["s"] * (ref.CALF_R1 - ref.CALF_R0)) + ref.HIP_R
        # 201 samples per segment: a neighbour of the true closest pair is at most half a step away on each segment
        step = 0.5 * (np.linalg.norm(foot - knee, axis=-1) + np.linalg.norm(h1 - h0, axis=-1)) / 200
        for i in list(rng.choice(len(d), 40, replace=False)) + [2000]:
            ds, _, _ = seg_dist(knee[i], foot[i], h0[i], h1[i])
            assert d[i] <= ds + 1e-12 and ds - d[i] <= step[i], (c["a"], c["b"], i, d[i], ds)


def test_hip_segment_of_the_twin(twin, cases):
    for c in cases:
        b, qb = c["b"], c["qb"]
        n = len(qb)
        org = np.ascontiguousarray(np.tile(ref.HIP_ORG[b], (n, 1)), dtype=np.float32)
        q0 = np.ascontiguousarray(qb[:, 0], dtype=np.float32); side = np.full(n, ref.SIDE[b], np.float32)
        h0, h1 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        assert twin.qa_selfcol_hip_segment_host(n, org.ctypes.data, q0.ctypes.data, side.ctypes.data, h0.ctypes.data, h1.ctypes.data) == 0
        assert np.abs(h0 - c["pts"][2]).max() < 1e-6 and np.abs(h1 - c["pts"][3]).max() < 1e-6


def test_gap_and_normal_against_float64(twin, cases):
    """fp32-rounded points in; ~20 fp32 operations on coordinates up to 0.5 m round to ~6e-7 m, the bound is 1e-5 m"""
    deep = touching = 0
    for c in cases:
        knee, foot, h0, h1 = c["pts"]
        out = run_lane(twin, knee, foot, h0, h1, True)
        assert np.isfinite(out["gap"]).all() and np.isfinite(out["n"]).all()
        assert np.abs(out["gap"] - c["gap"]).max() < 1e-5, (c["a"], c["b"], np.abs(out["gap"] - c["gap"]).max())
        d = c["gap"] + (ref.CALF_R0 + c["s"] * (ref.CALF_R1 - ref.CALF_R0)) + ref.HIP_R
        far = d > 1e-3
        assert np.abs(out["n"][far] - c["n"][far]).max() < 1e-4
        assert np.abs(np.linalg.norm(out["n"][far], axis=-1) - 1).max() < 1e-5
        deep += int((c["gap"] < -0.01).sum()); touching += int((np.abs(c["gap"]) < 0.01).sum())
    assert deep > 50 and touching > 50          # the set does hold contacts


def test_both_lanes_of_a_pair_agree_bit_for_bit(twin, cases):
    """swapping which leg is "first" (the calf's lane or the hip's lane evaluates): identical gap and parameters, negated normal"""
    for c in cases:
        knee, foot, h0, h1 = c["pts"]
        as_calf = run_lane(twin, knee, foot, h0, h1, True)
        as_hip = run_lane(twin, h0, h1, knee, foot, False)
        for k in ("gap", "s", "t"):
            assert np.array_equal(as_calf[k].view(np.uint32), as_hip[k].view(np.uint32)), k
        assert np.array_equal(as_calf["n"], -as_hip["n"])
        # each lane's own point lies on its own segment
        pc = knee + c["s"][:, None] * (foot - knee); ph = h0 + c["t"][:, None] * (h1 - h0)
        far = (c["gap"] + ref.HIP_R + ref.CALF_R0) > 1e-3
        assert np.abs(as_calf["p"] - pc)[far].max() < 2e-3 and np.abs(as_hip["p"] - ph)[far].max() < 2e-3     # closest points are ill-conditioned for near-parallel segments; the gap is not


# ------------------------------------------------------------------ host side
class _Recorder:
    def __init__(self):
        self.calls = []

    def set_self_collision_hips(self, on):
        self.calls.append(on)


def _bbc_cfg():
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = 8; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
    return cfg


def _tsc_cfg():
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    return Go2AgilityCfg()


@pytest.mark.parametrize("make", [_bbc_cfg, _tsc_cfg])
def test_config_flag_translation(make):
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import install_self_collision_hips
    cfg = make()
    assert cfg.asset.qa_self_collision_hips is False           # off by default: existing configs and goldens are untouched
    r = _Recorder()
    assert install_self_collision_hips(cfg, r) is False and r.calls == []
    cfg.asset.qa_self_collision_hips = True
    assert install_self_collision_hips(cfg, r) is True and r.calls == [True]
    with pytest.raises(NotImplementedError, match="qa_set_self_collision_hips"):
        install_self_collision_hips(cfg, object())
    cfg.asset.self_collisions = 1                              # the reference's flag: 1 = self-collision DISABLED
    with pytest.raises(ValueError, match="self_collisions"):
        install_self_collision_hips(cfg, _Recorder())


def test_bbc_env_installs_the_flag_before_anything_else_uses_the_engine():
    """LeggedRobot.__init__ hands the flag to the backend; the CPU oracle has no twin of it and is refused"""
    from quadrupedal_agility_amd.legged_gym.utils import get_args, task_registry
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import make_qa_config
    from tests.oracle_backend import OracleBackend

    class Backend(OracleBackend):
        def set_self_collision_hips(self, on):
            assert self.global_step == 0
            self.hips = on
    args = get_args(["--device", "cpu", "--num_envs", "8", "--self_collision_hips"])
    cfg = _bbc_cfg()
    env, cfg = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg, backend=Backend(make_qa_config(cfg, seed=1)))
    assert cfg.asset.qa_self_collision_hips is True and env.sim.hips is True and env.self_collision_hips is True
    cfg = _bbc_cfg()
    with pytest.raises(NotImplementedError, match="qa_set_self_collision_hips"):
        task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg, backend=OracleBackend(make_qa_config(cfg, seed=1)))
    cfg = _bbc_cfg()
    env, cfg = task_registry.make_env("go2_locomotion", args=get_args(["--device", "cpu", "--num_envs", "8"]), env_cfg=cfg,
                                      backend=OracleBackend(make_qa_config(cfg, seed=1)))
    assert env.self_collision_hips is False


def test_tsc_env_installs_the_flag():
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.oracle_backend import OracleBackend
    from tests.oracle_lib import load_oracle

    class Backend(OracleBackend):
        def set_self_collision_hips(self, on):
            self.hips = on
    kw = dict(sim_device="cpu", bookkeeping_lib=(load_oracle(), "qo_"))
    cfg = _tsc_cfg(); cfg.env.num_envs = 4; cfg.asset.qa_self_collision_hips = True
    env = lr.LeggedRobot(cfg, backend=Backend, **kw)
    assert env.sim.hips is True and env.self_collision_hips is True
    with pytest.raises(NotImplementedError, match="qa_set_self_collision_hips"):
        lr.LeggedRobot(cfg, backend=OracleBackend, **kw)


def test_command_line_switch_sets_the_config_in_both_trees():
    from quadrupedal_agility_amd.legged_gym.utils import helpers as bbc
    from quadrupedal_agility_amd.tsc.legged_gym.utils import helpers as tsc
    for mod, make in ((bbc, _bbc_cfg), (tsc, _tsc_cfg)):
        cfg, _ = mod.update_cfg_from_args(make(), None, mod.get_args(["--self_collision_hips"]))
        assert cfg.asset.qa_self_collision_hips is True
        cfg, _ = mod.update_cfg_from_args(make(), None, mod.get_args([]))
        assert cfg.asset.qa_self_collision_hips is False
    # train.py and play.py of both trees parse their command line with these get_args
    for rel in ("legged_gym/scripts/train.py", "legged_gym/scripts/play.py", "tsc/legged_gym/scripts/train.py", "tsc/legged_gym/scripts/play.py"):
        assert "get_args" in open(os.path.join(ROOT, "quadrupedal_agility_amd", rel)).read(), rel


def test_library_exports_the_entry_point_and_capi_binds_it():
    import __graft_entry__ as g
    g.build()
    lib = _capi.load_library()
    assert "set_self_collision_hips" in _capi.EXTENSION_SYMBOLS and "set_self_collision_hips" not in _capi.ABI_SYMBOLS
    f = lib.qa_set_self_collision_hips
    assert f.restype == C.c_int and len(f.argtypes) == 2
    assert f(None, 1) == -1                                        # QA_E_ARG: no handle (nothing touches the device)
    text = open(os.path.join(ROOT, "include", "qa_sim_selfcol.h")).read()
    assert "int qa_set_self_collision_hips(qa_sim *sim, int on);" in text and "BEFORE the first recording" in text
    from quadrupedal_agility_amd.sim import QaSim
    assert callable(QaSim.set_self_collision_hips)
